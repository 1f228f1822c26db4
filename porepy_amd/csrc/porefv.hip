// porefv.hip — C ABI (include/porefv.h) of the MI355X-native MPFA-O assembly + solve.
//
// Build (product):   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC porefv.hip
// Build (emulation): g++ -x c++ -DPFV_EMULATE -O2 -std=c++17 -shared -fPIC porefv.hip
//                    (test infrastructure; see backend.h)
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "fluxfn.h"
#include "isotherm.h"
#include "react.h"
namespace pfv {
static int rccl_exchange_halo(void* user, double* d_x, void* stream);  // rccl_hooks.inc
}
#include "topology.inc"
#include "mpfa_numeric.inc"
#include "linalg.inc"
#include "reorder.inc"
#include "dd.h"
#include "mpsa.inc"
#include "tpfa.inc"
#include "biot.inc"
#include "ad_flux.inc"
#include "upwind.inc"
#include "advdiff.inc"
#include "sweep.inc"
#include "flow_adjoint.inc"
#include "mpfa_adjoint.inc"
#include "advdiff_adjoint.inc"

namespace pfv {
#ifndef PFV_EMULATE
// stream triad a = b + s c (PFV_KERNEL_TRIAD): the measured device bandwidth next to the data-sheet figure
__global__ void __launch_bounds__(256) k_triad(int64_t n2, D2* __restrict__ a, const D2* __restrict__ b,
                                               const D2* __restrict__ c) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n2; i += 4 * stride) {
    D2 x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = b[i + u * stride];
      y[u] = c[i + u * stride];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      D2 r;
      r.x = x[u].x + 0.5 * y[u].x;
      r.y = x[u].y + 0.5 * y[u].y;
      a[i + u * stride] = r;
    }
  }
  for (; i < n2; i += stride) {
    D2 r;
    r.x = b[i].x + 0.5 * c[i].x;
    r.y = b[i].y + 0.5 * c[i].y;
    a[i] = r;
  }
}
// read-only stream (PFV_KERNEL_READ): sum of 2^28 doubles, 16 bytes per lane, four loads in flight; the sums go
// to a small array so that nothing is optimised away
__global__ void __launch_bounds__(256) k_read_stream(int64_t n2, const D2* __restrict__ b, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  for (; i + 3 * stride < n2; i += 4 * stride) {
    D2 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = b[i + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += x[u].x + x[u].y;
  }
  for (; i < n2; i += stride) acc += b[i].x + b[i].y;
  if (acc == 1.2345e300) out[0] = acc;  // (never true for the zero-filled buffer: keeps the loads alive)
}
#endif
pfv_ctx_impl::pfv_ctx_impl() = default;
pfv_ctx_impl::~pfv_ctx_impl() = default;
}  // namespace pfv

using pfv::be_d2h;
using pfv::be_h2d;
using pfv::Error;

namespace {

template <class F>
pfv_status guarded(pfv_ctx* h, F&& body) {
  if (!h) return PFV_ERR_ARGUMENT;
  pfv::PoolScope pool_scope(&h->pool);
  try {
#ifndef PFV_EMULATE
    PFV_HIP_CHECK(hipSetDevice(h->device));
#endif
    body();
    return PFV_OK;
  } catch (const Error& e) {
    h->err = e.what();
    return (pfv_status)e.status;
  } catch (const std::exception& e) {
    h->err = e.what();
    return PFV_ERR_HIP;
  }
}

void require(bool ok, const char* msg) {
  if (!ok) throw Error(PFV_ERR_ARGUMENT, msg);
}

bool pattern_ready(const pfv_ctx* h, int which) {
  if (which == PFV_MAT_USER_SYSTEM) return h->filled[which];
  if (which == PFV_MAT_TRANSPORT_SYSTEM) return h->have_transport;
  if (which == PFV_MAT_ADVDIFF_SYSTEM) return h->have_advdiff;
  if (which >= PFV_MAT_UPWIND && which <= PFV_MAT_UPWIND_RHS_NEU) return h->have_upwind;
  if (which == PFV_MAT_FLUX_JACOBIAN) return h->have_symbolic;
  return which >= PFV_MAT_STRESS ? h->have_mpsa_symbolic : h->have_symbolic;
}

template <class T>
void upload(pfv::Buf<T>& buf, const T* host, size_t n, pfv::stream_t s) {
  buf.ensure(n);
  be_h2d(buf.p, host, n * sizeof(T), s);
}

// what the setup of a hierarchy H (Amg, AmgNns) leaves in the statistics
template <class H>
void amg_setup_stats(pfv_ctx* h, const H& amg, int64_t levels, int64_t coarsest_rows, bool maps_reused) {
  h->stats.amg_setup_ms = amg.setup_ms;
  h->stats.amg_operator_complexity = amg.op_complexity;
  h->stats.amg_levels = levels;
  h->stats.amg_coarsest_rows = coarsest_rows;
  h->stats.amg_maps_reused = maps_reused ? 1 : 0;
}

}  // namespace

namespace {
// the leading rows of a pattern as a pattern of its own (shares the index arrays, frees nothing)
struct RowsView {
  pfv::CsrPattern V;
  RowsView(const pfv::CsrPattern& P, int64_t nrows) {
    V.nrows = nrows;
    V.ncols = P.ncols;
    V.nnz = P.nnz;  // (the window's entry positions index the full arrays)
    V.max_row = P.max_row;
    V.indptr.p = P.indptr.p;
    V.indices.p = P.indices.p;
  }
  ~RowsView() {
    V.indptr.p = nullptr;
    V.indices.p = nullptr;
  }
};
}  // namespace

extern "C" {

int pfv_is_device_build(void) {
#ifdef PFV_EMULATE
  return 0;
#else
  return 1;
#endif
}

pfv_status pfv_create(int device, pfv_ctx** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  pfv_ctx* h = nullptr;
  try {
    h = new pfv_ctx();
    h->device = device;
#ifndef PFV_EMULATE
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
      delete h;
      return PFV_ERR_HIP;  // no GPU: the product library never falls back to the host
    }
    if (device < 0 || device >= count) {
      delete h;
      return PFV_ERR_ARGUMENT;
    }
    PFV_HIP_CHECK(hipSetDevice(device));
    PFV_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = h->stream;
    PFV_HIP_CHECK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
#endif
  } catch (...) {
    delete h;
    return PFV_ERR_HIP;
  }
  *out = h;
  return PFV_OK;
}

void pfv_destroy(pfv_ctx* h) {
  if (!h) return;
#ifndef PFV_EMULATE
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
  }
  hipStream_t s = h->own_stream, s2 = h->aux_stream;
  if (s2) (void)hipStreamSynchronize(s2);
  {
    pfv::PoolScope pool_scope(&h->pool);
    delete h;
  }
  if (s) (void)hipStreamDestroy(s);
  if (s2) (void)hipStreamDestroy(s2);
#else
  {
    pfv::PoolScope pool_scope(&h->pool);
    delete h;
  }
#endif
}

const char* pfv_last_error(pfv_ctx* h) { return h ? h->err.c_str() : "null handle"; }

// right-hand-side / solution vectors of the assemble and solve calls: host memory by default, device
// memory after pfv_set_vectors_on_device(h, 1)
static void vec_in(pfv_ctx* h, double* dst, const double* src, size_t n) {
  if (h->vectors_on_device) pfv::be_d2d(dst, src, n * sizeof(double), h->stream);
  else be_h2d(dst, src, n * sizeof(double), h->stream);
}

// ... and the mirror for what the calls hand back (does not synchronise)
static void vec_out(pfv_ctx* h, double* dst, const double* src, size_t n) {
  if (h->vectors_on_device) pfv::be_d2d(dst, src, n * sizeof(double), h->stream);
  else be_d2h(dst, src, n * sizeof(double), h->stream);
}

// ---- the active system and the solver caches keyed on it ("The active system and its caches") ---------
// A call that makes a system the active one calls values_changed (when it wrote the values) and activate, and touches
// none of the fields behind them itself.

// is system `which` of the handle (a PFV_MAT_* selector with values of its own) the active one?
static bool active_is(const pfv_ctx* h, int which) { return h->active.valid && h->active.val == h->val[which].p; }

static void activate(pfv_ctx* h, const pfv::CsrPattern& P, double* val, double* diag, double* rhs, int64_t n, int bs,
                     bool is_grid) {
  h->active.P = &P;
  h->active.val = val;
  h->active.diag = diag;
  h->active.rhs = rhs;
  h->active.n = n;
  h->active_bs = bs;
  h->active_is_grid = is_grid;
  h->active.valid = true;
}

// what becomes of the SpMV windows (win_sys, win_rows: functions of a pattern, keyed on its index array) when the
// values of a system change
enum class Windows {
  keep,     // the pattern under the values is the one the windows were keyed on: a refresh of values in place
  consume,  // div @ flux assembled for a new discretization: a window the discretize call built for this very pattern
            // (win_*_prebuilt) survives once, any other is dropped
  drop,     // the pattern was rebuilt or replaced in buffers that keep their address: no window survives
};
// `drop` also clears the two win_*_prebuilt flags.  They are set by pfv_mpfa_discretize alone, together with the pointer
// they vouch for, and read by `consume` alone; with the pointer gone, consuming a set flag and consuming a cleared one
// both end at (flag cleared, pointer null) -- and a pointer that a solve of another system sets in between is not
// pat_A's, so the next solve of the flow system builds its window either way.

// The values of a system were written into buffers whose address the caches below are keyed on: drop all five.
// copy_only: solver_system has just renumbered the active system -- what was built on the loop's copy goes, what was
// built on the active system itself (amg_block) and the copy's own key stay.
static void values_changed(pfv_ctx* h, Windows w, bool copy_only = false) {
  if (h->amg) h->amg->valid = false;  // keyed on amg_for_val
  h->nns_stale = true;                // amg_nns, keyed on amg_nns_for_val
  if (h->block_pc) h->block_pc->for_val = nullptr;
  if (!copy_only) {
    if (h->amg_block) h->amg_block->valid = false;
    h->perm_for_val = nullptr;  // the renumbered copy
  }
  if (w == Windows::consume) {
    if (!h->win_sys_prebuilt) h->win_for = nullptr;
    if (!h->win_rows_prebuilt) h->win_rows_for = nullptr;
  } else if (w == Windows::drop) {
    h->win_for = h->win_rows_for = nullptr;
  }
  if (w != Windows::keep) h->win_sys_prebuilt = h->win_rows_prebuilt = false;
}

pfv_status pfv_set_vectors_on_device(pfv_ctx* h, int on) {
  return guarded(h, [&] { h->vectors_on_device = on != 0; });
}

pfv_status pfv_set_grid(pfv_ctx* h, int nd, int64_t nc, int64_t nf, int64_t nn, const double* nodes,
                        const int32_t* cf_indptr, const int32_t* cf_indices, const int8_t* cf_sign,
                        const int32_t* fn_indptr, const int32_t* fn_indices,
                        const double* face_normals, const double* face_centers,
                        const double* cell_centers, const double* face_areas) {
  return guarded(h, [&] {
    require(nd >= 1 && nd <= 3, "nd must be 1, 2 or 3 (1-D grids: TPFA only, as in the reference, mpfa.py:690-712)");
    require(nc > 0 && nf > 0 && nn > 0, "empty grid");
    require(nodes && cf_indptr && cf_indices && cf_sign && fn_indptr && fn_indices && face_normals &&
                face_centers && cell_centers && face_areas,
            "null grid array");
    require(nc < (int64_t(1) << 31) && nf < (int64_t(1) << 31) && nn < (int64_t(1) << 31), "grid too large for int32 ids");
    auto s = h->stream;
    pfv::be_sync(s);
    h->pool.trim();  // a new grid: the cached block sizes are of no use any more
    h->nd = nd;
    h->nc = nc;
    h->nf = nf;
    h->nn = nn;
    h->ncf = cf_indptr[nc];
    h->nsf = fn_indptr[nf];
    require(cf_indptr[0] == 0 && fn_indptr[0] == 0, "indptr must start at 0");
    for (int d = 0; d < 3; ++d) {
      double lo = face_centers[(size_t)d * nf], hi = lo;
      for (int64_t f = 1; f < nf; ++f) {
        const double x = face_centers[(size_t)d * nf + f];
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
      }
      h->bbox_lo[d] = lo;
      h->bbox_hi[d] = hi;
    }
    upload(h->nodes, nodes, 3 * (size_t)nn, s);
    upload(h->fnorm, face_normals, 3 * (size_t)nf, s);
    upload(h->fcen, face_centers, 3 * (size_t)nf, s);
    upload(h->ccen, cell_centers, 3 * (size_t)nc, s);
    ++h->grid_serial;  // (device-made near-null spaces follow the cell centres)
    upload(h->farea, face_areas, (size_t)nf, s);
    upload(h->cf_ptr, cf_indptr, (size_t)nc + 1, s);
    upload(h->cf_idx, cf_indices, (size_t)h->ncf, s);
    upload(h->cf_sgn, cf_sign, (size_t)h->ncf, s);
    upload(h->fn_ptr, fn_indptr, (size_t)nf + 1, s);
    upload(h->fn_idx, fn_indices, (size_t)h->nsf, s);
    h->have_grid = true;
    h->periodic = false;
    h->have_cell_order = false;
    h->perm_for_val = nullptr;
    h->win_for = h->win_rows_for = nullptr;
    h->have_topology = h->have_symbolic = h->have_numeric = h->have_system = false;
    h->topo_key = h->symb_key = 0;
    h->adj_map_key = 0;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
    h->biot_rows_complete = false;
    h->rows_complete = false;
    h->rows_complete_m = false;
    h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
    h->subface_bc = h->mpsa_subface_bc = false;
    h->tpfa_mode = false;
    h->have_mpsa_numeric = h->have_mpsa_symbolic = h->have_mech_system = false;
    h->active.valid = false;
    for (bool& f : h->filled) f = false;
    h->have_q_res = h->have_upw_bc = h->have_upwind = h->have_transport = h->have_pat_T = h->have_upw_cells = false;
    h->have_tpos_T = false;
    h->have_cmap = h->have_tpos_A = false;
    h->have_acc_t = h->have_src_t = false;
    h->transport_zero_diag = -1;
    h->have_advdiff = h->have_adv_bD = h->have_adv_acc = h->have_adv_src = false;
    h->advdiff_zero_diag = -1;
    h->sweep.reset();
    h->transport_q = nullptr;
  });
}

pfv_status pfv_set_periodic(pfv_ctx* h, const int32_t* native_cell, const double* shift) {
  return guarded(h, [&] {
    require(h->have_grid, "pfv_set_grid first");
    require((native_cell == nullptr) == (shift == nullptr), "give both arrays, or neither to clear");
    h->have_numeric = h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
    h->rows_complete = false;
    if (!native_cell) {
      h->periodic = false;
      return;
    }
    upload(h->face_native, native_cell, (size_t)h->nf, h->stream);
    upload(h->face_shift, shift, 3 * (size_t)h->nf, h->stream);
    h->periodic = true;
  });
}

pfv_status pfv_mpfa_set_params(pfv_ctx* h, const double* perm_33n, const uint8_t* bc_flags,
                               const double* robin_weight, double eta, const double* eta_subface) {
  return guarded(h, [&] {
    require(h->have_grid, "pfv_set_grid must be called first");
    require(perm_33n && bc_flags, "null parameter array");
    auto s = h->stream;
    upload(h->perm, perm_33n, 9 * (size_t)h->nc, s);
    upload(h->bcflag, bc_flags, (size_t)h->nf, s);
    if (robin_weight) {
      upload(h->robin, robin_weight, (size_t)h->nf, s);
    } else {
      std::vector<double> ones((size_t)h->nf, 1.0);
      upload(h->robin, ones.data(), ones.size(), s);
    }
    h->eta = eta;
    h->have_eta_sub = eta_subface != nullptr;
    if (eta_subface) upload(h->eta_sub, eta_subface, (size_t)h->nsf, s);
    h->have_params = true;
    h->subface_bc = false;
    h->have_numeric = h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
  });
}

pfv_status pfv_mpfa_set_permeability(pfv_ctx* h, const double* perm_33n) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_params, "pfv_mpfa_set_params first");
    require(perm_33n != nullptr, "null parameter array");
    h->perm.ensure(9 * (size_t)h->nc);
    vec_in(h, h->perm.p, perm_33n, 9 * (size_t)h->nc);
    h->have_numeric = h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
  });
}

pfv_status pfv_mpfa_set_subface_bc(pfv_ctx* h, const uint8_t* bc_flags_sub, const double* robin_weight_sub) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_params, "pfv_mpfa_set_params first");
    h->subface_bc = false;
    h->have_numeric = h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
    h->rows_complete = false;
    if (!bc_flags_sub) return;
    const size_t nsf = (size_t)h->nsf;
    upload(h->bcflag_s, bc_flags_sub, nsf, h->stream);
    if (robin_weight_sub) {
      upload(h->robin_s, robin_weight_sub, nsf, h->stream);
    } else {
      std::vector<double> ones(nsf, 1.0);
      upload(h->robin_s, ones.data(), nsf, h->stream);
    }
    h->subface_bc = true;
  });
}

namespace {
// A rebuilt topology (PFV_DISCR_REBUILD_TOPOLOGY, the timed step of bench.py) against the symbolic outputs the handle
// still holds: the patterns of the six matrices and of A, the column -> pair maps and the face records are functions of
// the topology alone.  When the digest of the topology just built equals the one they were built from (topology.inc:
// topology_digest; sizes are part of it) they are kept: nothing build_symbolic would write differs from what is there.
// The topology itself is ALWAYS rebuilt -- that is what the flag asks for, and what the digest is taken of; a miss (new
// grid, other boundary, first call) runs the symbolic phase as before.  PFV_SYMB_REUSE=0: never keep (the cold step).
// Ref: the phase this stands for is SubcellTopology + the index work of the SpGEMM chain, _fvutils.py:51-172.
bool symbolic_outputs_still_valid(pfv_ctx* h) {
  h->stats.symbolic_reused = 0;
  if (pfv::env_int("PFV_SYMB_REUSE", 1) == 0) {
    h->topo_key = 0;
    return false;
  }
  h->topo_key = pfv::topology_digest(*h);
  const bool keep = h->have_symbolic && !h->tpfa_mode && h->symb_key != 0 && h->symb_key == h->topo_key &&
                    h->pat_flux.nrows == h->nf && h->pat_A.nrows == h->nc;
  if (keep) {
    // what build_symbolic's prologue does for the VALUES: they belong to the previous discretization
    for (int m = PFV_MAT_FLUX; m <= PFV_MAT_SYSTEM; ++m) h->filled[m] = false;
    h->stats.symbolic_reused = 1;
  }
  return keep;
}
}  // namespace

pfv_status pfv_mpfa_discretize(pfv_ctx* h, uint32_t flags) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_params, "grid and parameters must be set before discretize");
    require(h->nd >= 2, "MPFA needs a 2-D or 3-D grid (1-D: pfv_tpfa_discretize)");
    auto s = h->stream;
    pfv::Timer tm, tall;
    tall.start(s);
    bool node_done = false;
    const bool with_vs = !(flags & PFV_DISCR_SKIP_VECTOR_SOURCE);
    if (!h->have_topology || !h->have_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) {
      tm.start(s);
      pfv::build_topology(*h);
      h->stats.topology_ms = tm.stop(s);
      tm.start(s);
      const bool keep_symbolic = symbolic_outputs_still_valid(h);
      if (keep_symbolic) {
        h->stats.symbolic_ms = tm.stop(s);  // (the digest and its read-back)
      } else {
#ifndef PFV_EMULATE
      // The symbolic phase (CSR patterns) and the interaction-region kernel (local inverses) both
      // depend on the sub-cell topology only, and both are bound by latency at low occupancy, not by
      // bandwidth: the node kernel goes to the handle's second stream and shares the CUs with the
      // symbolic kernels.  Its buffers live in the handle (nothing it touches passes through the block
      // cache while the other stream runs); the status words of the two phases are disjoint.
      if (h->aux_stream && pfv::env_int("PFV_OVERLAP_NODE", 1) != 0) {
        pfv::stream_t ns = h->aux_stream;
        pfv::StreamFork fork(s, ns);   // ns waits for everything enqueued on s so far
        pfv::Timer tn;
        tn.start(ns);
        pfv::launch_node_kernel(*h, nullptr, ns);
        tn.mark(ns);
        tm.start(s);
        pfv::build_symbolic(*h);
        h->stats.symbolic_ms = tm.stop(s);
        fork.join();                              // s waits for the node kernel
        h->stats.node_ms = tn.elapsed_after_sync();
        pfv::check_node_status(*h, s);
        node_done = true;
      }
#endif
      if (!node_done) {
        tm.start(s);
        pfv::build_symbolic(*h);
        h->stats.symbolic_ms = tm.stop(s);
      }
      h->tpfa_mode = false;
      h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
      }  // !keep_symbolic
    }
    if (!node_done) {
      tm.start(s);
      pfv::run_node_kernel(*h);
      h->stats.node_ms = tm.stop(s);
    }
    tm.start(s);
    if (h->subface_bc) {
      if (!h->have_sub_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) pfv::build_subface_symbolic(*h);
      pfv::run_subface_kernel(*h);
      if (with_vs) pfv::run_face_kernel(*h, true);
    } else {
#ifndef PFV_EMULATE
      // The SpMV window of A (spmv_win.inc) only needs A's pattern, which the symbolic phase has left:
      // when the solve is going to work on the system in place (grid numbered along the Morton curve),
      // it is built now on the second stream, beside the face kernel, instead of inside pfv_solve.
      h->win_sys_prebuilt = h->win_rows_prebuilt = false;
      const bool big = h->pat_A.nnz >= pfv::env_int("PFV_SPMV_WINDOW_MIN_NNZ", 20000);
      const bool prebuild = h->aux_stream && h->have_cell_order && h->cell_order_identity &&
                            pfv::env_int("PFV_OVERLAP_WINDOW", 1) != 0 && pfv::env_int("PFV_REORDER", 1) != 0 && big;
      // (a sharded solve multiplies the rows of the owned cells: the window of those rows, for the
      // number of owned rows of the previous solve on this handle)
      const bool prebuild_rows = !prebuild && h->aux_stream && h->win_rows_n > 0 && h->win_rows_n <= h->nc &&
                                 pfv::env_int("PFV_OVERLAP_WINDOW", 1) != 0 && big;
      if (prebuild || prebuild_rows) {
        pfv::StreamFork fork(s, h->aux_stream);
        pfv::run_face_kernel(*h, with_vs);
        h->stream = h->aux_stream;
        try {
          if (prebuild) {
            // the windows are a function of A's pattern alone: kept when the symbolic phase has just proved the
            // pattern equal to the one they were built for (sizes + checksum of the index arrays)
            const bool keep = h->win_sys.ok && h->pat_A_checksum != 0 && h->win_sys_checksum == h->pat_A_checksum &&
                              h->win_sys.nrows == h->pat_A.nrows && h->win_sys.nnz == h->pat_A.nnz &&
                              pfv::env_int("PFV_WIN_REUSE", 1) != 0;
            h->stats.win_reused = keep ? 1 : 0;
            if (!keep) {
              h->win_sys_checksum = 0;
              pfv::win_build(*h, h->pat_A, h->win_sys);
              if (h->win_sys.ok) h->win_sys_checksum = h->pat_A_checksum;
            }
          } else {
            // (the window of the owned rows of a sharded solve: kept like win_sys when A's pattern is proved equal)
            const bool keep = h->win_rows.ok && h->pat_A_checksum != 0 && h->win_rows_checksum == h->pat_A_checksum &&
                              h->win_rows.nrows == h->win_rows_n && pfv::env_int("PFV_WIN_REUSE", 1) != 0;
            h->stats.win_reused = keep ? 1 : 0;
            if (!keep) {
              h->win_rows_checksum = 0;
              RowsView rows(h->pat_A, h->win_rows_n);
              pfv::win_build(*h, rows.V, h->win_rows);
              if (h->win_rows.ok) h->win_rows_checksum = h->pat_A_checksum;
            }
          }
        } catch (...) {
          h->stream = s;
          throw;
        }
        h->stream = s;
        fork.join();
        if (prebuild) {
          h->win_for = h->pat_A.indices.p;
          h->win_sys_prebuilt = true;
        } else {
          h->win_rows_for = h->pat_A.indices.p;
          h->win_rows_prebuilt = true;
        }
      } else
#endif
      pfv::run_face_kernel(*h, with_vs);
    }
    h->stats.face_ms = tm.stop(s);
    h->stats.discretize_ms = tall.stop(s);
    h->have_numeric = true;
    h->rows_complete = !h->subface_bc;
    h->have_system = false;
    h->filled[PFV_MAT_SYSTEM] = false;
    double bytes = 0.0;
    bytes += 2.0 * 8.0 * (double)h->pat_flux.nnz + 2.0 * 8.0 * (double)h->pat_bound.nnz;
    if (with_vs) bytes += 2.0 * 8.0 * (double)h->pat_vs.nnz;
    h->stats.bytes_written_outputs = bytes;
  });
}

pfv_status pfv_tpfa_discretize(pfv_ctx* h, int vector_source_dim) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_params, "grid and parameters must be set before discretize");
    require(vector_source_dim >= 1 && vector_source_dim <= 3, "vector_source_dim must be 1, 2 or 3");
    auto s = h->stream;
    pfv::Timer tm;
    tm.start(s);
    h->have_symbolic = false;  // the MPFA patterns (if any) are replaced
    h->symb_key = 0;
    h->rows_complete = false;
    for (int m = PFV_MAT_FLUX; m <= PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE; ++m) h->filled[m] = false;
    h->filled[PFV_MAT_SYSTEM] = false;
    pfv::tpfa_discretize(*h, vector_source_dim);
    h->stats.face_ms = tm.stop(s);
    h->tpfa_mode = true;
    h->have_symbolic = true;
    h->have_topology = false;  // an MPFA call on this handle rebuilds its own topology + patterns
    h->have_numeric = true;
    h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
  });
}

pfv_status pfv_tpfa_transmissibility_ad(pfv_ctx* h, const double* perm_33n, double* t_face, double* dt_dk) {
  return guarded(h, [&] {
    require(h->have_grid, "the grid must be set first");
    require(perm_33n && t_face && dt_dk, "null argument");
    auto s = h->stream;
    const size_t nc = (size_t)h->nc, nf = (size_t)h->nf, ncf = (size_t)h->ncf;
    pfv::Buf<double> perm, t, jac;
    double* dp = perm.ensure(9 * nc);
    vec_in(h, dp, perm_33n, 9 * nc);
    double* dt = h->vectors_on_device ? t_face : t.ensure(std::max<size_t>(nf, 1));
    double* dj = h->vectors_on_device ? dt_dk : jac.ensure(std::max<size_t>(9 * ncf, 1));
    pfv::tpfa_transmissibility_ad(*h, dp, dt, dj);
    if (!h->vectors_on_device) {
      be_d2h(t_face, dt, sizeof(double) * nf, s);
      be_d2h(dt_dk, dj, sizeof(double) * 9 * ncf, s);
    } else {
      pfv::be_sync(s);
    }
  });
}

pfv_status pfv_mpfa_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces, const int32_t* faces,
                                     int keep_other_rows) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_params, "grid and parameters must be set before discretize");
    require(n_faces >= 0 && (n_faces == 0 || faces), "bad face list");
    require(h->nd >= 2, "MPFA needs a 2-D or 3-D grid");
    require(!h->subface_bc, "partial discretization with conditions per sub-face is not covered");
    require(!keep_other_rows || h->rows_complete,
            "update of a discretization that was never computed on this handle");
    for (int64_t i = 0; i < n_faces; ++i)
      require(faces[i] >= 0 && faces[i] < h->nf, "face index out of range");
    auto s = h->stream;
    pfv::Timer tm;
    if (!h->have_topology || !h->have_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) {
      require(!keep_other_rows, "the topology cannot be rebuilt under an update");
      h->tpfa_mode = false;
      tm.start(s);
      pfv::build_topology(*h);
      h->stats.topology_ms = tm.stop(s);
      tm.start(s);
      pfv::build_symbolic(*h);
      h->stats.symbolic_ms = tm.stop(s);
    }
    const bool with_vs = !(flags & PFV_DISCR_SKIP_VECTOR_SOURCE);
    int32_t* sub = h->face_subset.ensure(std::max<int64_t>(n_faces, 1));
    uint8_t* act = h->node_active.ensure(h->nn);
    pfv::be_h2d(sub, faces, sizeof(int32_t) * (size_t)n_faces, s);
    pfv::be_memset(act, 0, (size_t)h->nn, s);
    const int32_t* fn_ptr = h->fn_ptr;
    const int32_t* fn_idx = h->fn_idx;
    pfv::parallel_for(s, n_faces, PFV_LAMBDA(int64_t i) {
      const int f = sub[i];
      for (int e = fn_ptr[f]; e < fn_ptr[f + 1]; ++e) act[fn_idx[e]] = 1;
    });
    tm.start(s);
    pfv::run_node_kernel(*h, act);
    h->stats.node_ms = tm.stop(s);
    if (!keep_other_rows) {
      h->rows_complete = false;
      const int mats[6] = {PFV_MAT_FLUX, PFV_MAT_BOUND_FLUX, PFV_MAT_BOUND_PRESSURE_CELL,
                           PFV_MAT_BOUND_PRESSURE_FACE, PFV_MAT_VECTOR_SOURCE,
                           PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE};
      for (int m : mats) {
        if (m >= PFV_MAT_VECTOR_SOURCE && !with_vs) continue;
        const int64_t nnz = h->pattern_of(m).nnz;
        double* v = h->val[m].ensure(std::max<int64_t>(nnz, 1));
        pfv::be_memset(v, 0, sizeof(double) * (size_t)nnz, s);
      }
    }
    tm.start(s);
    pfv::run_face_kernel(*h, with_vs, sub, n_faces);
    h->stats.face_ms = tm.stop(s);
    h->have_numeric = true;
    h->have_system = false;
    h->win_sys_prebuilt = h->win_rows_prebuilt = false;
    h->filled[PFV_MAT_SYSTEM] = false;
  });
}

// index arrays that are written on first use (topology.inc: ensure_vs_indices)
static void materialize_pattern(pfv_ctx* h, int which) {
  if (which == PFV_MAT_VECTOR_SOURCE || which == PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE) pfv::ensure_vs_indices(*h);
}

pfv_status pfv_matrix_info(pfv_ctx* h, int which, int64_t* nrows, int64_t* ncols, int64_t* nnz) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS, "bad matrix selector");
    require(pattern_ready(h, which), "discretize first");
    const pfv::CsrPattern& P = h->pattern_of(which);
    if (nrows) *nrows = P.nrows;
    if (ncols) *ncols = P.ncols;
    if (nnz) *nnz = P.nnz;
  });
}

pfv_status pfv_get_matrix(pfv_ctx* h, int which, int32_t* indptr, int32_t* indices, double* data) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS, "bad matrix selector");
    require(pattern_ready(h, which), "discretize first");
    if ((which == PFV_MAT_VECTOR_SOURCE || which == PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE) && h->vs_implicit && !h->tpfa_mode)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "vector_source has more than 2^31 entries on this handle: int32 CSR arrays "
                                            "cannot hold it -- fetch it by rows (pfv_get_matrix_rows)");
    if (indices) materialize_pattern(h, which);
    const pfv::CsrPattern& P = h->pattern_of(which);
    auto s = h->stream;
    if (indptr) be_d2h(indptr, P.indptr.p, sizeof(int32_t) * (size_t)(P.nrows + 1), s);
    if (indices) be_d2h(indices, P.indices.p, sizeof(int32_t) * (size_t)P.nnz, s);
    if (data) {
      require(h->filled[which], "matrix values have not been computed");
      be_d2h(data, h->val[which].p, sizeof(double) * (size_t)P.nnz, s);
    }
  });
}

pfv_status pfv_get_matrix_rows(pfv_ctx* h, int which, int64_t n_rows, const int32_t* rows, int32_t* out_indptr,
                               int32_t* out_indices, double* out_data) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS, "bad matrix selector");
    require(pattern_ready(h, which), "discretize first");
    require(n_rows >= 0 && (n_rows == 0 || rows) && out_indptr, "bad row list");
    // (vector-source matrices beyond 2^31 entries: rows are expanded from the flux pattern, nd entries per flux entry)
    const bool imp = (which == PFV_MAT_VECTOR_SOURCE || which == PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE) && h->vs_implicit &&
                     !h->tpfa_mode;
    const int mult = imp ? h->nd : 1;
    if (!imp && (out_indices || out_data)) materialize_pattern(h, which);
    const pfv::CsrPattern& P = imp ? h->pat_flux : h->pattern_of(which);
    for (int64_t i = 0; i < n_rows; ++i) require(rows[i] >= 0 && rows[i] < P.nrows, "row index out of range");
    auto s = h->stream;
    pfv::Buf<int32_t> d_rows, d_len, d_ix;
    pfv::Buf<int64_t> d_ptr;
    pfv::Buf<double> d_val;
    int32_t* dr = d_rows.ensure(std::max<int64_t>(n_rows, 1));
    int32_t* dl = d_len.ensure(n_rows + 1);
    int64_t* dp = d_ptr.ensure(n_rows + 1);
    be_h2d(dr, rows, sizeof(int32_t) * (size_t)n_rows, s);
    const int32_t* ip = P.indptr;
    pfv::parallel_for(s, n_rows, PFV_LAMBDA(int64_t i) { dl[i] = (ip[dr[i] + 1] - ip[dr[i]]) * mult; });
    pfv::exclusive_scan<int32_t, int64_t>(s, h->scratch, dl, dp, (size_t)n_rows);
    std::vector<int64_t> hp((size_t)n_rows + 1);
    be_d2h(hp.data(), dp, sizeof(int64_t) * (size_t)(n_rows + 1), s);
    require(hp[(size_t)n_rows] < (int64_t(1) << 31), "more than 2^31 entries requested");
    for (int64_t i = 0; i <= n_rows; ++i) out_indptr[i] = (int32_t)hp[(size_t)i];
    if (!out_indices && !out_data) return;
    require(!out_data || h->filled[which], "matrix values have not been computed");
    const int64_t tot = hp[(size_t)n_rows];
    const int32_t* ix = P.indices;
    const double* val = out_data ? h->val[which].p : nullptr;
    int32_t* tix = d_ix.ensure(std::max<int64_t>(tot, 1));
    double* tv = d_val.ensure(std::max<int64_t>(out_data ? tot : 1, 1));
    pfv::wave_for<16>(s, n_rows, 0, PFV_LAMBDA(const pfv::WaveCtx& w) {
      const int64_t i = w.item;
      const int p0 = ip[dr[i]], len = dl[i];
      const int64_t o = dp[i];
      if (mult == 1) {
        PFV_LANES(k, len) {
          tix[o + k] = ix[p0 + k];
          if (val) tv[o + k] = val[p0 + k];
        }
      } else {
        PFV_LANES(k, len) {
          const int e = k / mult, cpt = k - e * mult;
          tix[o + k] = ix[p0 + e] * mult + cpt;
          if (val) tv[o + k] = val[(int64_t)p0 * mult + k];
        }
      }
    });
    if (out_indices) be_d2h(out_indices, tix, sizeof(int32_t) * (size_t)tot, s);
    if (out_data) be_d2h(out_data, tv, sizeof(double) * (size_t)tot, s);
  });
}

pfv_status pfv_mpfa_assemble(pfv_ctx* h, const double* bc_values, const double* vector_source,
                             const double* source) {
  return guarded(h, [&] {
    require(h->have_numeric, "discretize first");
    require(!h->subface_bc, "flux has sub-face rows (conditions per sub-face): collapse it before assembling");
    require(bc_values != nullptr, "bc_values is required");
    require(!vector_source || h->filled[PFV_MAT_VECTOR_SOURCE], "vector_source matrix was skipped");
    auto s = h->stream;
    pfv::Timer tm;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc;
    const size_t nvs = (size_t)h->pat_vs.ncols;  // nd (MPFA) or ambient-dimension (TPFA) entries per cell
    double* in = h->vec_in.ensure(nf + nvs + nc);
    double* d_bc = in;
    double* d_vs = vector_source ? in + nf : nullptr;
    double* d_src = source ? in + nf + nvs : nullptr;
    vec_in(h, d_bc, bc_values, nf);
    if (d_vs) vec_in(h, d_vs, vector_source, nvs);
    if (d_src) vec_in(h, d_src, source, nc);
    tm.start(s);
    if (!h->have_system) {
      pfv::assemble_system(*h);
      h->have_advdiff = h->have_adv_bD = false;  // (advdiff.inc: built on the previous div @ flux)
      values_changed(h, Windows::consume);
    }
    pfv::assemble_rhs(*h, d_bc, d_vs, d_src);
    h->stats.assemble_ms = tm.stop(s);
    h->have_system = true;
    h->have_flow_rhs = true;
    activate(h, h->pat_A, h->val[PFV_MAT_SYSTEM].p, h->diag.p, h->rhs.p, h->nc, 1, true);
  });
}

pfv_status pfv_mpfa_ad_flux_system(pfv_ctx* h, const double* p, const double* dk_dp, const double* bc_values,
                                   const double* vector_source, const double* source, double* flux_out,
                                   uint32_t flags) {
  return guarded(h, [&] {
    require(h->have_numeric && !h->tpfa_mode, "pfv_mpfa_discretize first");
    require(!h->subface_bc, "conditions per sub-face are not covered");
    require(p != nullptr, "p is required");
    require(!vector_source || h->filled[PFV_MAT_VECTOR_SOURCE], "vector_source matrix was skipped");
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc, nvs = (size_t)h->pat_vs.ncols;
    pfv::Buf<double> in_;
    double* in = in_.ensure(nc + 9 * nc + nf + nvs + nc + nf);
    double* d_p = in;
    double* d_dk = dk_dp ? in + nc : nullptr;
    double* d_bc = bc_values ? in + 10 * nc : nullptr;
    double* d_vs = vector_source ? in + 10 * nc + nf : nullptr;
    double* d_src = source ? in + 10 * nc + nf + nvs : nullptr;
    double* d_q = in + 11 * nc + nf + nvs;
    vec_in(h, d_p, p, nc);
    if (d_dk) vec_in(h, d_dk, dk_dp, 9 * nc);
    if (d_bc) vec_in(h, d_bc, bc_values, nf);
    if (d_vs) vec_in(h, d_vs, vector_source, nvs);
    if (d_src) vec_in(h, d_src, source, nc);
    pfv::Timer tm;
    tm.start(s);
    pfv::ad_flux_system(*h, d_p, d_dk, d_bc, d_vs, d_src, flux_out ? d_q : nullptr,
                        (flags & PFV_AD_WANT_FLUX_JACOBIAN) != 0);
    h->stats.assemble_ms = tm.stop(s);
    if (flux_out) vec_out(h, flux_out, d_q, nf);
    pfv::be_sync(s);
    h->have_system = false;  // PFV_MAT_SYSTEM now holds J, not div flux: pfv_mpfa_assemble rebuilds it
    values_changed(h, Windows::drop);
    activate(h, h->pat_A, h->val[PFV_MAT_SYSTEM].p, h->diag.p, h->rhs.p, h->nc, 1, true);
  });
}

// ---- upwind advection and the transport step (upwind.inc) ------------------------------------------------------
static void upwind_supported(pfv_ctx* h) {
  require(h->have_grid, "pfv_set_grid first");
  if (h->periodic) throw pfv::Error(PFV_ERR_UNSUPPORTED, "upwind on periodic grids is not covered");
  if (h->shard) throw pfv::Error(PFV_ERR_UNSUPPORTED, "the transport calls have no sharded form");
}

// the transport system no longer belongs to the discretization on the handle: it must not stay the active system
// (keep_order: the discretization and its flux stay, only the assembled values go -- pfv_transport_advance_multi)
static void upwind_drop_transport(pfv_ctx* h, bool keep_order = false) {
  if (h->have_transport && active_is(h, PFV_MAT_TRANSPORT_SYSTEM)) h->active.valid = false;
  h->have_transport = false;
  h->filled[PFV_MAT_TRANSPORT_SYSTEM] = false;
  h->transport_zero_diag = -1;
  if (!keep_order && h->sweep && h->sweep->for_system == PFV_MAT_TRANSPORT_SYSTEM) h->sweep->valid = false;
}

// An assembly of system `which` with the flux d_q: a flow order built for another system, or for a flux with other
// edges, is stale.  Costs nothing unless a sweep solve has built an order on this handle.
static void sweep_note_assembly(pfv_ctx* h, int which, const double* d_q) {
  if (!h->sweep || !h->sweep->valid) return;
  if (h->sweep->for_system != which || !pfv::sweep_same_edges(*h, *h->sweep, d_q)) h->sweep->valid = false;
}

static bool transport_is_active(const pfv_ctx* h) {
  return h->have_transport && active_is(h, PFV_MAT_TRANSPORT_SYSTEM);
}

pfv_status pfv_mpfa_face_flux(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                              double* q_out) {
  return guarded(h, [&] {
    upwind_supported(h);
    require(h->have_numeric && h->filled[PFV_MAT_FLUX] && h->filled[PFV_MAT_BOUND_FLUX], "discretize the flow first");
    if (h->subface_bc)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "flux has sub-face rows (conditions per sub-face): no face flux");
    require(p && bc_values, "p and bc_values are required");
    require(!vector_source || h->filled[PFV_MAT_VECTOR_SOURCE], "vector_source matrix was skipped");
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc, nvs = (size_t)h->pat_vs.ncols;
    pfv::Buf<double> in_;
    double* in = in_.ensure(nc + nf + nvs);
    double* d_p = in;
    double* d_bc = in + nc;
    double* d_vs = vector_source ? in + nc + nf : nullptr;
    vec_in(h, d_p, p, nc);
    vec_in(h, d_bc, bc_values, nf);
    if (d_vs) vec_in(h, d_vs, vector_source, nvs);
    pfv::Timer tm;
    tm.start(s);
    pfv::upwind_face_flux(*h, d_p, d_bc, d_vs);
    h->stats.face_flux_ms = tm.stop(s);
    h->have_q_res = true;
    if (q_out) vec_out(h, q_out, h->q_res.p, nf);
    pfv::be_sync(s);  // (the staging buffer is freed on return)
  });
}

pfv_status pfv_upwind_set_bc(pfv_ctx* h, const uint8_t* bc_flags) {
  return guarded(h, [&] {
    upwind_supported(h);
    h->have_upw_bc = bc_flags != nullptr;
    if (bc_flags) upload(h->upw_bc, bc_flags, (size_t)h->nf, h->stream);
    upwind_drop_transport(h);
    h->have_upwind = false;
  });
}

// the flux argument of the upwind calls: the caller's array staged into `stage`, or the fallback when it is NULL
static const double* upwind_flux_in(pfv_ctx* h, const double* q, pfv::Buf<double>& stage) {
  if (!q) return nullptr;
  double* d = stage.ensure((size_t)h->nf);
  vec_in(h, d, q, (size_t)h->nf);
  return d;
}

pfv_status pfv_upwind_discretize(pfv_ctx* h, const double* q, int num_components) {
  return guarded(h, [&] {
    upwind_supported(h);
    require(num_components >= 1, "num_components must be at least 1");
    require(q || h->have_q_res, "no face flux given and no resident face flux on the handle (pfv_mpfa_face_flux)");
    auto s = h->stream;
    const double* d_q = upwind_flux_in(h, q, h->q_t);
    if (!d_q) d_q = h->q_res.p;
    upwind_drop_transport(h);
    h->have_upwind = false;
    for (int m = PFV_MAT_UPWIND; m <= PFV_MAT_UPWIND_RHS_NEU; ++m) h->filled[m] = false;
    pfv::Timer tm;
    tm.start(s);
    pfv::upwind_discretize(*h, d_q, num_components);
    h->stats.upwind_ms = tm.stop(s);
    h->upw_ncomp = num_components;
    h->have_upwind = true;
  });
}

pfv_status pfv_upwind_assemble(pfv_ctx* h, const double* q, const double* bc_values, const double* accumulation,
                               const double* c_old, const double* source, double* bound_rhs_out) {
  return guarded(h, [&] {
    upwind_supported(h);
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "Dimension mismatch in assembly of discretization term: upwinding with multiple "
                               "components only discretizes");
    require(bc_values != nullptr, "bc_values is required");
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc;
    const double* d_q = upwind_flux_in(h, q, h->q_t);
    if (!d_q) d_q = h->upw_q.p;
    double* d_bc = h->bc_t.ensure(nf);
    vec_in(h, d_bc, bc_values, nf);
    h->have_acc_t = accumulation != nullptr;
    h->have_src_t = source != nullptr;
    if (accumulation) vec_in(h, h->acc_t.ensure(nc), accumulation, nc);
    if (source) vec_in(h, h->src_t.ensure(nc), source, nc);
    const double* d_cold = nullptr;
    if (c_old) {
      vec_in(h, h->c_t.ensure(nc), c_old, nc);
      d_cold = h->c_t.p;
    }
    pfv::Timer tm;
    tm.start(s);
    pfv::upwind_assemble(*h, d_q, d_bc, h->have_acc_t ? h->acc_t.p : nullptr, d_cold,
                         h->have_src_t ? h->src_t.p : nullptr);
    h->stats.transport_assemble_ms = tm.stop(s);
    h->transport_q = d_q;
    sweep_note_assembly(h, PFV_MAT_TRANSPORT_SYSTEM, d_q);
    if (bound_rhs_out) vec_out(h, bound_rhs_out, h->bref_t.p, nc);
    pfv::be_sync(s);
    h->have_transport = true;
    values_changed(h, Windows::drop);
    activate(h, h->pat_T, h->val[PFV_MAT_TRANSPORT_SYSTEM].p, h->diag_t.p, h->rhs_t.p, h->nc, 1, true);
  });
}

// ---- what the step calls share ----------------------------------------------------------------------------------------
// The flow order of the flux d_q on the transport system, in the caller's numbering and with its launch plan: built on
// first use and kept while the flux brings the same edges; the time of a rebuild is added to order_ms.  same_flux: d_q is
// the flux the order was last checked against in this call (an assembly in between can only have dropped it).
static pfv::Sweep& transport_order(pfv_ctx* h, const double* d_q, double& order_ms, bool same_flux = false) {
  if (!h->sweep) h->sweep = std::make_unique<pfv::Sweep>();
  if (!same_flux) sweep_note_assembly(h, PFV_MAT_TRANSPORT_SYSTEM, d_q);
  pfv::Sweep& sw = *h->sweep;
  if (!sw.valid) {
    pfv::sweep_build_order(*h, sw, d_q, PFV_MAT_TRANSPORT_SYSTEM);
    order_ms += sw.order_ms;
  }
  pfv::sweep_set_numbering(*h, sw, false);
  pfv::sweep_make_plan(sw);
  return sw;
}

// The policy of the core loop: iterate() until the core has settled, at most maxit times.  The stop test runs every
// kNlCoreCheck-th iteration and at maxit: stop_test() launches it, ONE host read brings `out` into hst, judge() says
// whether the core has settled.
struct CoreRun {
  int iterations = 0;
  bool settled = false;
};
static CoreRun core_iterate(pfv_ctx* h, int maxit, const double* out, std::vector<double>& hst,
                            const std::function<void()>& iterate, const std::function<void()>& stop_test,
                            const std::function<bool()>& judge) {
  CoreRun run;
  while (run.iterations < maxit && !run.settled) {
    iterate();
    ++run.iterations;
    if (run.iterations % pfv::kNlCoreCheck != 0 && run.iterations != maxit) continue;
    stop_test();
    be_d2h(hst.data(), out, sizeof(double) * hst.size(), h->stream);
    run.settled = judge();
  }
  return run;
}

// the sweep statistics of a step call; launches < 0: those of the launch plan
static void sweep_step_stats(pfv_ctx* h, int64_t launches, double order_ms) {
  if (!h->sweep || !h->sweep->valid) return;
  pfv::sweep_make_plan(*h->sweep);
  h->stats.sweep_levels = h->sweep->nlev;
  h->stats.sweep_core_cells = h->sweep->n_core;
  h->stats.sweep_launches = launches >= 0 ? launches : (int64_t)h->sweep->plan.size();
  h->stats.sweep_order_ms = order_ms;
}

// The error of a failed step (status st, text err) is what the call reports, whatever the epilogue (st2) did.
static pfv_status step_status(pfv_ctx* h, pfv_status st, const std::string& err, pfv_status st2) {
  if (st == PFV_OK) return st2;
  h->err = err;
  return st;
}

// ---- the set-up and the frame of the flow-ordered step calls: the three forward ones and the four adjoints ---------------
struct StepSetup {
  std::unique_ptr<pfv::Timer> tm;  // running from transport_system on
  bool touched = false;            // the transport system on the handle is the call's
  double order_ms = 0.0;
};

// The system of a step call, with the timer started: A = div diag(q) U without accumulation (its diagonal: the outflow
// of the cell), once per call; own_rows: what the call checks or prepares on A's rows; then the flow order, unless the
// call may do without one.  (The boundary term that upwind_assemble forms beside A is not used: every call has its own.)
static void transport_system(pfv_ctx* h, StepSetup& S, const double* d_q, const double* d_bc,
                             const std::function<void()>& own_rows = nullptr, bool order = true) {
  S.tm = std::make_unique<pfv::Timer>();
  S.tm->start(h->stream);
  upwind_drop_transport(h, true);
  S.touched = true;
  pfv::upwind_assemble(*h, d_q, d_bc, nullptr, nullptr, nullptr);
  values_changed(h, Windows::drop);
  if (own_rows) own_rows();
  if (order) transport_order(h, d_q, S.order_ms);
}

// the set-up of a call: its checks, its uploads, transport_system, its work buffers.  A set-up that fails leaves no system
// behind (A without accumulation: not a system to be solved with).
static pfv_status step_setup(pfv_ctx* h, StepSetup& S, int32_t* steps_done, const std::function<void()>& body) {
  if (steps_done) *steps_done = 0;
  const pfv_status st = guarded(h, body);
  if (st != PFV_OK && S.touched) upwind_drop_transport(h, true);
  return st;
}

struct StepRun {
  int32_t completed = 0;  // the steps accepted
  int64_t core_total = 0, launches = 0;
  double ms = 0.0;
  std::vector<pfv_solve_info> info;
  std::vector<double> hst;  // the norms of the last host read
};

// The end of a call whose steps ended in (st, err): the timer stopped into run.ms, the call's outputs(st), the transport
// system dropped; *steps_done.  The error of a failed step is what the call reports, whatever happens here.
static pfv_status step_finish(pfv_ctx* h, StepSetup& S, StepRun& run, pfv_status st, const std::string& err,
                              int32_t* steps_done, const std::function<void(pfv_status)>& outputs) {
  const pfv_status st2 = guarded(h, [&] {
    run.ms = S.tm->stop(h->stream);
    S.tm.reset();
    outputs(st);
    pfv::be_sync(h->stream);
    upwind_drop_transport(h, true);
  });
  if (steps_done) *steps_done = run.completed;
  return step_status(h, st, err, st2);
}

// The frame of a call after its set-up: body(step) for step = 0 .. n_steps - 1 until one fails, then step_finish.
// body returns PFV_OK, having counted run.completed, or the verdict of a refused step with its text in h->err.
static pfv_status step_frame(pfv_ctx* h, StepSetup& S, StepRun& run, int n_steps, int32_t* steps_done,
                             const std::function<pfv_status(int)>& body,
                             const std::function<void(pfv_status)>& outputs) {
  pfv_status st = PFV_OK;
  for (int step = 0; step < n_steps && st == PFV_OK; ++step) {
    pfv_status verdict = PFV_OK;
    st = guarded(h, [&] { verdict = body(step); });
    if (st == PFV_OK) st = verdict;
  }
  return step_finish(h, S, run, st, st != PFV_OK ? h->err : std::string(), steps_done, outputs);
}

// ---- the step loop of pfv_transport_advance and pfv_advdiff_advance --------------------------------------------------
struct StepLoop {  // what differs between the two
  pfv::Buf<double> pfv::pfv_ctx_impl::*state;  // the state between the steps
  pfv::Buf<double> pfv::pfv_ctx_impl::*keep;   // the state before the step, for a second attempt
  void (*step_rhs)(pfv::pfv_ctx_impl&, const double*);
  bool jacobi_unless_sweep;  // the transport matrix is one-sided: any other choice on the handle is replaced by Jacobi
  bool jacobi_fallback;      // a step the AMG- or sweep-preconditioned solve gives up on: again with Jacobi-GMRES
};
struct StepHooks {  // what the adjoint loop (pfv_advdiff_adjoint) adds; the forward calls pass none
  std::function<void(int)> rhs;    // instead of StepLoop::step_rhs: the right-hand side of step `step` from the state
  std::function<void(int)> after;  // after an accepted step, the state holding its solution
};
struct StepTotals {
  bool ran = false;  // the checks passed: the totals below are to be written to the statistics
  int64_t iterations = 0, gmres_retries = 0, precond_fallbacks = 0, direct = 0, direct_fallbacks = 0;
  double order_ms = 0.0, ms = 0.0;
};

// `checks` throws for what the call does not take.  Then n_steps times: form the right-hand side, solve from the state;
// a step that ends in NaN under BiCGStab is solved again with GMRES from the kept state.  BiCGStab can break down
// (rho = (r_hat, r) = 0: the residual turns NaN) where the first residual sits in cells nothing flows back into --
// injection into a field at rest, the matrix of an acyclic flow being triangular.  The error of a failed step is what
// pfv_last_error reports, whatever the epilogue does.
static pfv_status advance_steps(pfv_ctx* h, const StepLoop& L, const std::function<void()>& checks, int n_steps,
                                int method, double rtol, int maxit, double* c, int32_t* steps_done,
                                pfv_solve_info* last, StepTotals& tot, const StepHooks* hooks = nullptr) {
  if (steps_done) *steps_done = 0;
  std::unique_ptr<pfv::Timer> tm;
  pfv_status st = guarded(h, [&] {
    checks();
    if (c) vec_in(h, (h->*L.state).ensure((size_t)h->nc), c, (size_t)h->nc);
    else pfv::be_memset((h->*L.state).ensure((size_t)h->nc), 0, sizeof(double) * (size_t)h->nc, h->stream);  // (hooks)
    tm = std::make_unique<pfv::Timer>();
    tm->start(h->stream);
  });
  if (st != PFV_OK) return st;
  tot.ran = true;
  pfv::Buf<double>&state = h->*L.state, &keep = h->*L.keep;
  const bool caller_on_device = h->vectors_on_device;
  const int precond = h->precond;
  h->vectors_on_device = true;  // the state stays on the device between the steps
  if (L.jacobi_unless_sweep && precond != PFV_PRECOND_SWEEP) h->precond = PFV_PRECOND_JACOBI;
  const size_t nbytes = (size_t)h->nc * sizeof(double);
  const bool keep_state = method == PFV_SOLVE_BICGSTAB || L.jacobi_fallback;
  auto restore_state = [&] { return guarded(h, [&] { pfv::be_d2d(state.p, keep.p, nbytes, h->stream); }); };
  auto solve = [&](int m, pfv_solve_info& info) {
    const pfv_status r = pfv_solve(h, m, rtol, maxit, 0, state.p, state.p, &info);
    tot.iterations += info.iterations;
    return r;
  };
  for (int step = 0; step < n_steps && st == PFV_OK; ++step) {
    st = guarded(h, [&] {
      if (hooks && hooks->rhs) hooks->rhs(step);
      else L.step_rhs(*h, state.p);
      if (keep_state) pfv::be_d2d(keep.ensure((size_t)h->nc), state.p, nbytes, h->stream);
    });
    if (st != PFV_OK) break;
    pfv_solve_info info{};
    st = solve(method, info);
    tot.direct += h->stats.sweep_direct_steps;
    tot.direct_fallbacks += h->stats.sweep_direct_fallbacks;
    tot.order_ms += h->stats.sweep_order_ms;
    if (st == PFV_ERR_NOT_CONVERGED && method == PFV_SOLVE_BICGSTAB && !(info.rel_residual == info.rel_residual)) {
      if ((st = restore_state()) != PFV_OK) break;
      ++tot.gmres_retries;
      st = solve(PFV_SOLVE_GMRES, info);
      tot.direct += h->stats.sweep_direct_steps;
      tot.direct_fallbacks += h->stats.sweep_direct_fallbacks;
    }
    if (st == PFV_ERR_NOT_CONVERGED && L.jacobi_fallback && (precond == PFV_PRECOND_AMG || precond == PFV_PRECOND_SWEEP)) {
      if ((st = restore_state()) != PFV_OK) break;
      ++tot.precond_fallbacks;
      h->precond = PFV_PRECOND_JACOBI;
      st = solve(PFV_SOLVE_GMRES, info);
      h->precond = precond;
    }
    if (last) *last = info;
    if (st == PFV_OK && hooks && hooks->after) st = guarded(h, [&] { hooks->after(step); });
    if (st == PFV_OK && steps_done) ++*steps_done;
  }
  h->vectors_on_device = caller_on_device;
  h->precond = precond;
  const std::string err = h->err;
  const pfv_status st2 = guarded(h, [&] {
    tot.ms = tm->stop(h->stream);
    tm.reset();
    if (c) vec_out(h, c, state.p, (size_t)h->nc);
    pfv::be_sync(h->stream);
  });
  return step_status(h, st, err, st2);
}

pfv_status pfv_transport_advance(pfv_ctx* h, int n_steps, int method, double rtol, int maxit, double* c,
                                 int32_t* steps_done, pfv_solve_info* last) {
  static const StepLoop loop{&pfv_ctx::c_t, &pfv_ctx::c_keep, pfv::upwind_step_rhs, true, false};
  StepTotals tot;
  const pfv_status st = advance_steps(h, loop, [&] {
    upwind_supported(h);
    require(transport_is_active(h), "pfv_upwind_assemble first (the transport system must be the active one)");
    require(n_steps >= 0 && c != nullptr, "bad argument");
    require(method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES (the transport matrix is not symmetric)");
  }, n_steps, method, rtol, maxit, c, steps_done, last, tot);
  if (tot.ran) {
    h->stats.transport_advance_ms = tot.ms;
    h->stats.transport_iterations = tot.iterations;
    h->stats.transport_gmres_retries = tot.gmres_retries;
    h->stats.sweep_direct_steps = tot.direct;
    h->stats.sweep_direct_fallbacks = tot.direct_fallbacks;
    h->stats.sweep_order_ms = tot.order_ms;
  }
  return st;
}

// ---- k components on one flux -----------------------------------------------------------------------------------------
// Fast path (PFV_PRECOND_SWEEP, acyclic flux): per step one right-hand side, one sweep and one residual check for all
// components, in the caller's numbering on pat_T, one host read of 2k numbers.  Everything else -- another
// preconditioner, a cyclic core, a component whose check fails -- is pfv_upwind_assemble + pfv_transport_advance on
// that component's arrays, which lie on the device component by component as the caller passed them.
static std::string zero_diagonal_text(int64_t zd, int k) {  // zd: what upwind_zero_diag_multi found
  return "zero diagonal entry in row " + std::to_string(zd / k) + ", component " + std::to_string(zd % k) +
         " of the transport system (a cell without outflow and without an accumulation term): the solvers do not apply";
}

// Component by component: component_steps(a, steps, done) takes component a `steps` steps from mc_x to mc_z.  Should one
// stop early, all are taken again from the start to the step it reached, so that c is one state of all components.
// Returns the first failure with its text in err; completed: the step all have reached, their state in mc_x.
using MultiComponent = std::function<pfv_status(int, int, int32_t&)>;
static pfv_status multi_by_component(pfv_ctx* h, int k, int n_steps, const MultiComponent& component_steps,
                                     int32_t& completed, std::string& err) {
  pfv_status st = PFV_OK;
  int target = n_steps;
  for (;;) {
    int32_t least = target;
    for (int a = 0; a < k; ++a) {
      int32_t done = 0;
      const pfv_status r = component_steps(a, target, done);
      if (r == PFV_OK) continue;
      if (st == PFV_OK) {
        st = r;
        err = h->err;
      }
      least = std::min(least, done);
      break;
    }
    if (least == target) break;
    target = least;
  }
  completed = target;
  if (target > 0) h->mc_x.swap(h->mc_z);
  return st;
}

pfv_status pfv_transport_advance_multi(pfv_ctx* h, const double* q, int n_comp, const double* bc_values,
                                       const double* accumulation, const double* source, int n_steps, int method,
                                       double rtol, int maxit, double* c, int32_t* steps_done, pfv_solve_info* last) {
  const int k = n_comp;
  StepSetup S;
  bool fast = false;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the components share one discretization: pfv_upwind_discretize with num_components = 1");
    require(n_comp >= 1 && n_comp <= 64, "n_comp must lie in 1 .. 64");
    require(bc_values && accumulation && c, "bc_values, accumulation and c are required");
    require(n_steps >= 0, "bad argument");
    require(method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES (the transport matrix is not symmetric)");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)nc * k >= (int64_t(1) << 31) || (int64_t)nf * k >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "n_comp x cells (faces) beyond int32 indices");
    if (q) vec_in(h, h->mc_q.ensure(nf), q, nf);
    vec_in(h, h->mc_bc.ensure(k * nf), bc_values, k * nf);
    vec_in(h, h->mc_acc.ensure(k * nc), accumulation, k * nc);
    if (source) vec_in(h, h->mc_src.ensure(k * nc), source, k * nc);
    vec_in(h, h->mc_c.ensure(k * nc), c, k * nc);
    d_q = q ? h->mc_q.p : h->upw_q.p;
    const bool sweep = h->precond == PFV_PRECOND_SWEEP;  // (any other preconditioner: no order is built)
    transport_system(h, S, d_q, h->mc_bc.p, [&] {
      pfv::multi_interleave(*h, (int64_t)nc, k, h->mc_acc.p, h->mc_acc_i.ensure(k * nc));
      if (source) pfv::multi_interleave(*h, (int64_t)nc, k, h->mc_src.p, h->mc_src_i.ensure(k * nc));
      pfv::multi_interleave(*h, (int64_t)nc, k, h->mc_c.p, h->mc_x.ensure(k * nc));
      h->mc_z.ensure(k * nc);
      h->mc_r.ensure(k * nc);
      h->mc_col.ensure(nc);
      h->mc_nrm.ensure(2 * (size_t)k);
      const int64_t zd = pfv::upwind_zero_diag_multi(*h, k, h->diag_t.p, h->mc_acc_i.p);
      if (zd >= 0) throw Error(PFV_ERR_UNSUPPORTED, zero_diagonal_text(zd, k));
      pfv::upwind_bref_multi(*h, k, d_q, h->mc_bc.p, h->mc_bref_i.ensure(k * nc));
    }, sweep);
    fast = sweep && h->sweep->n_core == 0;
  });
  if (st != PFV_OK) return st;

  const bool caller_on_device = h->vectors_on_device;
  const double* src_i = source ? h->mc_src_i.p : nullptr;
  int64_t direct_steps = 0, fallback = 0, iterations = 0, retries = 0;
  StepRun run;
  run.info.assign((size_t)k, pfv_solve_info{});
  // `steps` steps of component a alone, from mc_x to mc_z, as pfv_upwind_assemble + pfv_transport_advance do them
  const MultiComponent component_steps = [&](int a, int steps, int32_t& done) {
    done = 0;
    pfv_status r = guarded(h, [&] { pfv::multi_get_column(*h, (int64_t)nc, k, a, h->mc_x.p, h->mc_col.p); });
    if (r != PFV_OK) return r;
    h->vectors_on_device = true;
    r = pfv_upwind_assemble(h, q ? h->mc_q.p : nullptr, h->mc_bc.p + (size_t)a * nf, h->mc_acc.p + (size_t)a * nc,
                            nullptr, source ? h->mc_src.p + (size_t)a * nc : nullptr, nullptr);
    if (r == PFV_OK) {
      r = pfv_transport_advance(h, steps, method, rtol, maxit, h->mc_col.p, &done, &run.info[(size_t)a]);
      iterations += h->stats.transport_iterations;
      retries += h->stats.transport_gmres_retries;
      S.order_ms += h->stats.sweep_order_ms;
    }
    h->vectors_on_device = caller_on_device;
    if (r != PFV_OK) return r;
    return guarded(h, [&] { pfv::multi_set_column(*h, (int64_t)nc, k, a, h->mc_col.p, h->mc_z.p); });
  };
  const auto outputs = [&](pfv_status) {
    pfv::multi_deinterleave(*h, (int64_t)nc, k, h->mc_x.p, h->mc_c.p);
    vec_out(h, c, h->mc_c.p, k * nc);
  };
  if (fast) {
    bool shared_values = true;  // PFV_MAT_TRANSPORT_SYSTEM holds A without accumulation
    st = step_frame(h, S, run, n_steps, steps_done, [&](int) -> pfv_status {
      if (!shared_values) {
        upwind_drop_transport(h, true);
        pfv::upwind_assemble(*h, d_q, h->mc_bc.p, nullptr, nullptr, nullptr);
        values_changed(h, Windows::drop);
        shared_values = true;
      }
      // (a component's own solve in between works in the renumbered system, and its assembly can drop the order)
      const pfv::Sweep& sw = transport_order(h, d_q, S.order_ms, true);
      const double* val = h->val[PFV_MAT_TRANSPORT_SYSTEM].p;
      run.hst.resize(2 * (size_t)k);
      pfv::upwind_step_rhs_multi(*h, k, h->mc_acc_i.p, src_i, h->mc_bref_i.p, h->mc_x.p, h->mc_r.p);
      pfv::sweep_apply_multi(*h, sw, h->pat_T, val, h->diag_t.p, h->mc_acc_i.p, k, h->mc_r.p, h->mc_z.p);
      pfv::sweep_residual_norms_multi(*h, h->pat_T, val, h->mc_acc_i.p, k, h->mc_r.p, h->mc_z.p, h->mc_nrm.p);
      be_d2h(run.hst.data(), h->mc_nrm.p, sizeof(double) * 2 * (size_t)k, h->stream);
      // The acceptance is this call's own: a right-hand side that is zero counts as converged whatever the sweep left,
      // and a component whose check fails is not refused but solved alone, from the state at the start of the step.
      int failed = 0;
      for (int a = 0; a < k; ++a) {
        const double bb = run.hst[(size_t)a], rr = run.hst[(size_t)k + a];
        pfv_solve_info& ia = run.info[(size_t)a];
        ia = pfv_solve_info{};
        ia.iterations = 1;
        if (!(bb > 0.0)) {  // r_a = 0 -> the sweep has left 0
          ia.converged = bb == 0.0 ? 1 : 0;
        } else {
          ia.rel_residual = std::sqrt(rr / bb);
          ia.converged = rr <= rtol * rtol * bb ? 1 : 0;
        }
        if (ia.converged) {
          ++iterations;
          continue;
        }
        ++failed;
        ++fallback;
        shared_values = false;
        int32_t done = 0;
        const pfv_status r = component_steps(a, 1, done);
        if (r != PFV_OK) return r;
      }
      h->mc_x.swap(h->mc_z);
      ++run.completed;
      if (!failed) ++direct_steps;
      return PFV_OK;
    }, outputs);
  } else {
    std::string err;
    st = multi_by_component(h, k, n_steps, component_steps, run.completed, err);
    fallback = (int64_t)k * run.completed;
    st = step_finish(h, S, run, st, err, steps_done, outputs);
  }
  if (last) {
    for (int a = 0; a < k; ++a) {
      last[a] = run.info[(size_t)a];
      if (fast && last[a].solve_ms == 0.0 && run.completed > 0) last[a].solve_ms = run.ms / run.completed;
    }
  }
  h->stats.transport_advance_ms = run.ms;
  h->stats.transport_iterations = iterations;
  h->stats.transport_gmres_retries = retries;
  h->stats.transport_multi_components = k;
  h->stats.transport_multi_direct_steps = direct_steps;
  h->stats.transport_multi_fallback_components = fallback;
  h->stats.sweep_direct_steps = direct_steps;
  if (h->precond == PFV_PRECOND_SWEEP) sweep_step_stats(h, -1, S.order_ms);
  return st;
}

// ---- what the input-check kernels found, as the error of the call ---------------------------------------------------
// off[m]: the lowest offender of check m, or kNoOffender.  The checks are judged in their order.  by_component: one bit
// per check of a [k][n] array, whose offender is named by item and component; skip: one bit per check whose array the
// caller has put a stand-in for (the adjoints have no state to be checked).
constexpr int32_t kNoOffender = 0x7f7f7f7f;
static void inputs_refused(const int32_t* off, int n_checks, const char* const* what, unsigned by_component, int k,
                           unsigned skip) {
  for (int m = 0; m < n_checks; ++m) {
    if ((skip >> m & 1u) || off[m] == kNoOffender) continue;
    if (by_component >> m & 1u)
      throw Error(PFV_ERR_ARGUMENT, what[m] + std::to_string(off[m] / k) + ", component " + std::to_string(off[m] % k));
    throw Error(PFV_ERR_ARGUMENT, what[m] + std::to_string(off[m]));
  }
}
constexpr unsigned kNlStates = 1u << 2 | 1u << 6;  // s and c of sweep_nl_check_inputs
static void nl_inputs_refused(const int32_t (&off)[pfv::kNlChecks], int k, unsigned skip = 0) {
  static const char* const what[pfv::kNlChecks] = {
      "accumulation must be positive: cell ", "negative sink in cell ", "s outside [0, 1] in cell ",
      "Dirichlet inflow value outside [0, 1] on face ", pfv::kUnmarkedInflowFace,
      "sorption must not be negative: cell ", "c is not finite in cell ", "c_bc_values is not finite on face "};
  inputs_refused(off, pfv::kNlChecks, what, 7u << 5, k, skip);
}
constexpr unsigned kReactState = 1u << 2;  // c of sweep_react_check_inputs
static void react_inputs_refused(const int32_t (&off)[pfv::kReactChecks], int k, unsigned skip = 0) {
  static const char* const what[pfv::kReactChecks] = {
      "accumulation must be positive: cell ", "rate_weight must not be negative: cell ", "c is not finite in cell ",
      "bc_values is not finite on face ", pfv::kUnmarkedInflowFace};
  inputs_refused(off, pfv::kReactChecks, what, 1u << 0 | 1u << 2 | 1u << 3, k, skip);
}

// ---- the saturation step: q f(s) in flow order (sweep.inc: sweep_row_nl) -----------------------------------------------
// Per step: rhs, the forward levels, the core level iterated by nonlinear Jacobi (a host read every kNlCoreCheck-th
// iteration), the backward levels, F(s) over all rows and ONE host read of its norms and the status words.  The state
// of the step's start stays in its own buffer until the step is accepted.
//   With k > 0 components carried by the phase (pfv_transport_advance_nl_multi; k == 0: pfv_transport_advance_nl) the
// same launches take them (sweep_row_nlc), the core iterates them jointly and the one host read brings their norms too.
// nl_out: [0, 4) the saturation's norms (all rows, core rows), [4] the two status words, [5, 5 + 2k) the components'
// (rhs_a, rhs_a) and (F_a, F_a) over all rows, [5 + 2k, 5 + 4k) the same over the core rows.
static pfv_status advance_nl(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params, int n_params,
                             const double* bc_values, const double* accumulation, const double* source,
                             const double* sink, int k, const double* c_bc_values, const double* sorption,
                             const double* c_source, int n_steps, double rtol, int maxit, double* s, double* cc,
                             int32_t* steps_done, pfv_solve_info* last) {
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv::FluxFn F;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    if (h->subface_bc) throw Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the saturation step needs pfv_upwind_discretize with num_components = 1");
    const std::string bad = pfv::fluxfn_check(fluxfn_kind, fluxfn_params, n_params);
    if (!bad.empty()) throw Error(PFV_ERR_ARGUMENT, bad);
    require(bc_values && accumulation && s, "bc_values, accumulation and s are required");
    require(k == 0 || (c_bc_values && cc), "c_bc_values and c are required");
    require(n_steps >= 0, "bad argument");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if (k > 0 && (int64_t)(k + 1) * (int64_t)std::max(nc, nf) >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "(k + 1) x cells (faces) beyond int32 indices");
    if (q) vec_in(h, h->nl_q.ensure(nf), q, nf);
    vec_in(h, h->nl_bc.ensure(nf), bc_values, nf);
    vec_in(h, h->nl_acc.ensure(nc), accumulation, nc);
    if (source) vec_in(h, h->nl_src.ensure(nc), source, nc);
    if (sink) vec_in(h, h->nl_sink.ensure(nc), sink, nc);
    vec_in(h, h->nl_s.ensure(nc), s, nc);
    if (k > 0) {  // component-major, as they came
      vec_in(h, h->nlc_cbc.ensure(k * nf), c_bc_values, k * nf);
      if (sorption) vec_in(h, h->nlc_ads_in.ensure(k * nc), sorption, k * nc);
      if (c_source) vec_in(h, h->nlc_src_in.ensure(k * nc), c_source, k * nc);
      vec_in(h, h->nlc_c_in.ensure(k * nc), cc, k * nc);
    }
    d_q = q ? h->nl_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    int32_t off[pfv::kNlChecks];
    pfv::sweep_nl_check_inputs(*h, d_q, h->nl_bc.p, h->nl_acc.p, sink ? h->nl_sink.p : nullptr, h->nl_s.p, k,
                               sorption ? h->nlc_ads_in.p : nullptr, h->nlc_c_in.p, h->nlc_cbc.p, off);
    nl_inputs_refused(off, k);
    if (fluxfn_kind == PFV_FLUXFN_TABLE)
      be_h2d(h->nl_table.ensure((size_t)n_params), fluxfn_params, sizeof(double) * (size_t)n_params, h->stream);
    F = pfv::fluxfn_make(fluxfn_kind, fluxfn_params, n_params, h->nl_table.p);
    transport_system(h, S, d_q, h->nl_bc.p, [&] {
      pfv::upwind_bref_nl(*h, F, d_q, h->nl_bc.p, h->nl_bref.ensure(nc));
      for (pfv::Buf<double>* b : {&h->nl_s2, &h->nl_phi, &h->nl_phi2, &h->nl_rhs, &h->nl_t}) b->ensure(nc);
      h->nl_out.ensure(8 + 4 * (size_t)k);
      if (k == 0) return;
      // the vectors of the step, cell-major interleaved
      if (sorption) pfv::multi_interleave(*h, (int64_t)nc, k, h->nlc_ads_in.p, h->nlc_ads.ensure(k * nc));
      if (c_source) pfv::multi_interleave(*h, (int64_t)nc, k, h->nlc_src_in.p, h->nlc_src.ensure(k * nc));
      pfv::multi_interleave(*h, (int64_t)nc, k, h->nlc_c_in.p, h->nlc_x.ensure(k * nc));
      pfv::upwind_bref_nlc(*h, F, k, d_q, h->nl_bc.p, h->nlc_cbc.p, h->nlc_bref.ensure(k * nc));
      for (pfv::Buf<double>* b : {&h->nlc_z, &h->nlc_psi, &h->nlc_psi2, &h->nlc_rhs, &h->nlc_t}) b->ensure(k * nc);
    });
    const pfv::Sweep& sw = *h->sweep;
    if (sw.n_core > 0) {
      h->nl_cb.ensure((size_t)sw.n_core);
      h->nl_ct.ensure((size_t)sw.n_core);
      if (k > 0) {
        h->nlc_cb.ensure(k * (size_t)sw.n_core);
        h->nlc_ct.ensure(k * (size_t)sw.n_core);
      }
    }
  });
  if (st != PFV_OK) return st;

  const double* d_src = source ? h->nl_src.p : nullptr;
  const double* d_sink = sink ? h->nl_sink.p : nullptr;
  StepRun run;  // (the solve of the step is this call's own: the saturation's info beside the components' in cinfo)
  pfv_solve_info info{};
  std::vector<pfv_solve_info> cinfo((size_t)k);
  std::vector<double>& hst = run.hst;
  hst.resize(5 + 4 * (size_t)k);
  st = step_frame(h, S, run, n_steps, steps_done, [&](int step) -> pfv_status {
    pfv::pfv_ctx_impl& c = *h;
    const pfv::Sweep& sw = *c.sweep;
    const double* val = c.val[PFV_MAT_TRANSPORT_SYSTEM].p;
    const double* diag = c.diag_t.p;
    const double *acc = c.nl_acc.p, *rhs = c.nl_rhs.p, *s_old = c.nl_s.p;
    double *s_new = c.nl_s2.p, *phi = c.nl_phi.p, *out = c.nl_out.p;
    int32_t* status = reinterpret_cast<int32_t*>(out + 4);  // [0] the levels outside the core, [1] the core
    const bool has_core = sw.n_core > 0;
    const int core = has_core ? sw.core_level : sw.nlev;
    pfv::NlComp C;  // the levels outside the core; Cc: the core level, with psi of the previous iterate
    if (k > 0) {
      C.k = k;
      C.ads = sorption ? c.nlc_ads.p : nullptr;
      C.rhs = c.nlc_rhs.p;
      C.c_start = c.nlc_x.p;
      C.c = c.nlc_z.p;
      C.psi = c.nlc_psi.p;
    }
    pfv::NlComp Cc = C;
    Cc.psi_prev = k > 0 ? c.nlc_psi2.p : nullptr;
    double* cout = out + 5;
    pfv::upwind_step_rhs_multi(c, 1, acc, d_src, c.nl_bref.p, s_old, c.nl_rhs.p);
    if (k > 0)
      pfv::upwind_step_rhs_nlc(c, k, acc, s_old, C.ads, c_source ? c.nlc_src.p : nullptr, c.nlc_bref.p, c.nlc_x.p,
                               c.nlc_rhs.p);
    pfv::be_memset(out, 0, 4 * sizeof(double), c.stream);
    pfv::be_memset(status, 0x7f, 2 * sizeof(int32_t), c.stream);
    if (k > 0) pfv::be_memset(cout, 0, 4 * (size_t)k * sizeof(double), c.stream);
    run.launches = pfv::sweep_apply_nl(c, sw, 0, core, c.pat_T, val, diag, d_sink, acc, rhs, F, s_old, s_new, phi, status,
                                       C);
    auto flagged = [&](bool core_too, int32_t& cell) {
      int32_t w[2];
      std::memcpy(w, hst.data() + 4, sizeof(w));
      cell = core_too ? std::min(w[0], w[1]) : w[0];
      return cell != 0x7f7f7f7f;
    };
    int core_it = 0;
    if (has_core) {
      pfv::sweep_residual_norms(c, c.nc, rhs, rhs, out);  // out[0] = (rhs, rhs)
      pfv::sweep_nl_core_init(c, sw, F, s_old, s_new, phi);
      if (k > 0) {
        pfv::sweep_norms_interleaved(c, c.nc, k, C.rhs, C.rhs, cout);  // cout[a] = (rhs_a, rhs_a)
        pfv::sweep_nlc_core_init(c, sw, phi, C);
      }
      const CoreRun cr = core_iterate(h, maxit, out, hst, [&] {
        // (once the saturation has passed its own test it stays, with its status word: the components alone go on)
        if (!Cc.frozen) pfv::sweep_nl_core_keep(c, sw, phi, c.nl_phi2.p, status + 1);
        if (k > 0) pfv::sweep_core_copy(c, sw, k, C.psi, c.nlc_psi2.p);
        pfv::sweep_levels_nl(c, sw, core, core + 1, c.pat_T, val, diag, d_sink, acc, rhs, F, s_new, c.nl_phi2.p, s_new,
                             phi, status + 1, Cc);
      }, [&] {
        if (!Cc.frozen) {
          pfv::sweep_nl_core_image(c, sw, c.pat_T, val, d_sink, acc, rhs, s_new, phi, c.nl_cb.p, c.nl_ct.p);
          pfv::sweep_residual_norms(c, sw.n_core, c.nl_cb.p, c.nl_ct.p, out + 2);  // out[3] = (F_core, F_core)
        }
        if (k > 0) {
          pfv::sweep_nlc_core_image(c, sw, c.pat_T, val, d_sink, acc, s_new, C, c.nlc_cb.p, c.nlc_ct.p);
          pfv::sweep_norms_interleaved(c, sw.n_core, k, c.nlc_cb.p, c.nlc_ct.p, cout + 2 * k);
        }
      }, [&] {
        bool settled = hst[3] <= 0.25 * rtol * rtol * hst[0];
        Cc.frozen = settled;
        for (int a = 0; a < k; ++a)  // (F_core_a, F_core_a) against (rhs_a, rhs_a)
          settled = settled && hst[5 + 3 * (size_t)k + a] <= 0.25 * rtol * rtol * hst[5 + (size_t)a];
        return settled;
      });
      core_it = cr.iterations;
      run.core_total += core_it;
      run.launches += 2;
      if (!cr.settled) {  // (what the backward levels would compute from this core is not judged)
        info = pfv_solve_info{};
        info.iterations = core_it;
        info.rel_residual = hst[0] > 0.0 ? std::sqrt(hst[3] / hst[0]) : 0.0;
        for (int a = 0; a < k; ++a) {
          const double bb = hst[5 + (size_t)a], rr = hst[5 + 3 * (size_t)k + a];
          cinfo[(size_t)a] = pfv_solve_info{};
          cinfo[(size_t)a].iterations = core_it;
          cinfo[(size_t)a].rel_residual = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
        }
        int32_t cell;  // (the core's word belongs to an iterate that has not settled: the other levels' alone)
        if (flagged(false, cell))
          throw Error(PFV_ERR_ARGUMENT, "step " + std::to_string(step) + " leaves [0, 1]: no root in cell " +
                                            std::to_string(cell));
        c.err = "step " + std::to_string(step) + ": the cyclic core of " + std::to_string(sw.n_core) +
                " cells did not settle in " + std::to_string(core_it) + " iterations";
        return PFV_ERR_NOT_CONVERGED;
      }
      run.launches += pfv::sweep_apply_nl(c, sw, core + 1, sw.nlev, c.pat_T, val, diag, d_sink, acc, rhs, F, s_old, s_new,
                                          phi, status, C);
    }
    if (k > 0) pfv::sweep_nlc_image(c, c.pat_T, val, d_sink, acc, s_new, phi, c.nl_t.p, C, c.nlc_t.p);
    else pfv::sweep_nl_image(c, c.pat_T, val, d_sink, acc, s_new, phi, c.nl_t.p);
    pfv::sweep_residual_norms(c, c.nc, rhs, c.nl_t.p, out);
    if (k > 0) pfv::sweep_norms_interleaved(c, c.nc, k, C.rhs, c.nlc_t.p, cout);
    be_d2h(hst.data(), out, sizeof(double) * hst.size(), c.stream);
    info = pfv_solve_info{};
    info.iterations = has_core ? core_it : 1;
    info.rel_residual = hst[0] > 0.0 ? std::sqrt(hst[1] / hst[0]) : 0.0;
    int32_t cell;
    if (flagged(true, cell))
      throw Error(PFV_ERR_ARGUMENT, "step " + std::to_string(step) + " leaves [0, 1]: no root in cell " +
                                        std::to_string(cell));
    info.converged = hst[1] <= rtol * rtol * hst[0] ? 1 : 0;
    int bad = info.converged ? -1 : k;  // the first component whose check fails; k: the saturation
    for (int a = k - 1; a >= 0; --a) {
      const double bb = hst[5 + (size_t)a], rr = hst[5 + (size_t)k + a];
      pfv_solve_info& ia = cinfo[(size_t)a];
      ia = pfv_solve_info{};
      ia.iterations = info.iterations;
      ia.rel_residual = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
      ia.converged = rr <= rtol * rtol * bb ? 1 : 0;  // (0 <= 0: a component that is absent everywhere is valid)
      if (!ia.converged && info.converged) bad = a;
    }
    if (bad >= 0) {
      const double rel = bad == k ? info.rel_residual : cinfo[(size_t)bad].rel_residual;
      c.err = "step " + std::to_string(step) + ": relative residual " + std::to_string(rel) +
              (bad == k ? std::string() : " of component " + std::to_string(bad)) +
              " after the sweep (a flux that contradicts the discretization's?)";
      return PFV_ERR_NOT_CONVERGED;
    }
    c.nl_s.swap(c.nl_s2);
    if (k > 0) c.nlc_x.swap(c.nlc_z);
    ++run.completed;
    return PFV_OK;
  }, [&](pfv_status) {
    vec_out(h, s, h->nl_s.p, nc);
    if (k > 0) {
      pfv::multi_deinterleave(*h, (int64_t)nc, k, h->nlc_x.p, h->nlc_c_in.p);
      vec_out(h, cc, h->nlc_c_in.p, k * nc);
    }
  });
  if (last) {
    *last = info;
    if (run.completed > 0) last->solve_ms = run.ms / run.completed;
    for (int a = 0; a < k; ++a) {
      last[1 + a] = cinfo[(size_t)a];
      last[1 + a].solve_ms = last->solve_ms;
    }
  }
  h->stats.transport_nl_ms = run.ms;
  h->stats.transport_nl_steps = run.completed;
  h->stats.transport_nl_core_iterations = run.core_total;
  h->stats.transport_nl_components = k;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

pfv_status pfv_transport_advance_nl(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                    int n_params, const double* bc_values, const double* accumulation,
                                    const double* source, const double* sink, int n_steps, double rtol, int maxit,
                                    double* s, int32_t* steps_done, pfv_solve_info* last) {
  return advance_nl(h, q, fluxfn_kind, fluxfn_params, n_params, bc_values, accumulation, source, sink, 0, nullptr,
                    nullptr, nullptr, n_steps, rtol, maxit, s, nullptr, steps_done, last);
}

pfv_status pfv_transport_advance_nl_multi(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                          int n_params, const double* bc_values, const double* accumulation,
                                          const double* source, const double* sink, int k, const double* c_bc_values,
                                          const double* sorption, const double* c_source, int n_steps, double rtol,
                                          int maxit, double* s, double* c, int32_t* steps_done, pfv_solve_info* last) {
  if (k < 1 || k > 64) {
    if (steps_done) *steps_done = 0;
    return guarded(h, [&] { require(false, "k must lie in 1 .. 64"); });
  }
  return advance_nl(h, q, fluxfn_kind, fluxfn_params, n_params, bc_values, accumulation, source, sink, k, c_bc_values,
                    sorption, c_source, n_steps, rtol, maxit, s, c, steps_done, last);
}

// ---- the solve of one step by a sweep: pfv_transport_advance_react, pfv_transport_advance_sorb and the four adjoints ------
// The levels before the core, the core level iterated by Jacobi on its rows (a host read every kNlCoreCheck-th
// iteration), the levels after it, the residual norms of all rows and ONE host read; then the acceptance.  A forward
// step walks the levels from first to last, an adjoint step from last to first.  The calls differ in their rows and
// their norms:
struct SweepWay {
  bool ascending;                       // the levels from first to last; otherwise from last to first
  const char *step_word, *sweep_word;  // what the messages call the step and the sweep
};
constexpr SweepWay kForwardSweep{true, "step ", "sweep"}, kAdjointSweep{false, "adjoint step ", "transposed sweep"};
struct SweepSolve {
  int pairs;        // of norms in out: (scale_a, scale_a) for all a, then (residual_a, residual_a)
  int saturation;   // sweep_accept's
  const double* out;
  SweepWay way;     // kForwardSweep or kAdjointSweep: every call names its own
  std::function<int64_t(int, int)> levels;  // the levels [from, to) in the call's direction; returns its launches
  std::function<void()> core_start;         // the unknowns of the core before the first iteration
  std::function<void()> core_step;          // one iteration on the core: the copy, then its rows
  std::function<void(bool)> norms;          // into out: of the core's rows only, or of all
  // A word behind the norms that the kernels set to an index (kNoOffender: not set), and what it means for step n: a
  // verdict, or an Error thrown.  flag_ends_core: the word says that the input admits no solution -- it ends the core's
  // iteration and is judged before anything else; otherwise it is judged on the finished sweep, before the acceptance.
  std::function<pfv_status(int, int32_t)> flagged;
  bool flag_ends_core = false;
};

// info from hst: (scale_a, scale_a), (residual_a, residual_a)
static void component_info(std::vector<pfv_solve_info>& info, const std::vector<double>& hst, int k, int it) {
  for (int a = 0; a < k; ++a) {
    const double bb = hst[(size_t)a], rr = hst[(size_t)k + a];
    info[(size_t)a] = pfv_solve_info{};
    info[(size_t)a].iterations = it;
    info[(size_t)a].rel_residual = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
  }
}

// ||residual_a|| <= tol ||scale_a|| for every component (0 <= 0 counts)
static bool norms_pass(const std::vector<double>& hst, int k, double tol) {
  bool pass = true;
  for (int a = 0; a < k; ++a) pass = pass && hst[(size_t)k + a] <= tol * tol * hst[(size_t)a];
  return pass;
}

// the acceptance of step n from the pairs of norms in hst (after component_info): the first component whose check fails
// is named; the saturation's, where there is one, before any component's
static pfv_status sweep_accept(pfv_ctx* h, const SweepSolve& V, std::vector<pfv_solve_info>& info,
                               const std::vector<double>& hst, double rtol, int n) {
  int bad = -1;
  for (int a = V.pairs - 1; a >= 0; --a) {
    info[(size_t)a].converged = hst[(size_t)V.pairs + a] <= rtol * rtol * hst[(size_t)a] ? 1 : 0;  // (0 <= 0 counts)
    if (!info[(size_t)a].converged) bad = a;
  }
  if (V.saturation >= 0 && !info[(size_t)V.saturation].converged) bad = V.saturation;
  if (bad < 0) return PFV_OK;
  h->err = V.way.step_word + std::to_string(n) + ": relative residual " + std::to_string(info[(size_t)bad].rel_residual) +
           (bad == V.saturation ? std::string() : " of component " + std::to_string(bad)) + " after the " +
           V.way.sweep_word + " (a flux that contradicts the discretization's?)";
  return PFV_ERR_NOT_CONVERGED;
}

// -> PFV_OK or the verdict of a refused step n (its text in h->err); it fills run.info and run.hst and counts
// run.launches (of this step) and run.core_total.  The core has settled at half the tolerance of the acceptance.
static pfv_status sweep_step_solve(pfv_ctx* h, const SweepSolve& V, StepRun& run, double rtol, int maxit, int n) {
  pfv::pfv_ctx_impl& cx = *h;
  const pfv::Sweep& sw = *cx.sweep;
  const int K = V.pairs;
  std::vector<double>& hst = run.hst;
  hst.resize(2 * (size_t)K + (V.flagged ? 1 : 0));
  auto flag = [&] {
    int32_t w = kNoOffender;
    if (V.flagged) std::memcpy(&w, hst.data() + 2 * K, sizeof(w));
    return w;
  };
  const bool has_core = sw.n_core > 0;
  const int core = has_core ? sw.core_level : V.way.ascending ? sw.nlev : -1;
  run.launches = V.way.ascending ? V.levels(0, core) : V.levels(core + 1, sw.nlev);
  int core_it = 0;
  if (has_core) {
    V.core_start();
    const CoreRun cr = core_iterate(h, maxit, V.out, hst, V.core_step, [&] { V.norms(true); }, [&] {
      return (V.flag_ends_core && flag() != kNoOffender) || norms_pass(hst, K, 0.5 * rtol);
    });
    core_it = cr.iterations;
    run.core_total += core_it;
    run.launches += 2;
    if (V.flag_ends_core && flag() != kNoOffender) return V.flagged(n, flag());
    if (!cr.settled) {  // (what the levels after the core would compute from it is not judged)
      component_info(run.info, hst, K, core_it);
      cx.err = V.way.step_word + std::to_string(n) + ": the cyclic core of " + std::to_string(sw.n_core) +
               " cells did not settle in " + std::to_string(core_it) + " iterations";
      return PFV_ERR_NOT_CONVERGED;
    }
    run.launches += V.way.ascending ? V.levels(core + 1, sw.nlev) : V.levels(0, core);
  }
  V.norms(false);
  be_d2h(hst.data(), V.out, sizeof(double) * hst.size(), cx.stream);
  if (V.flag_ends_core && flag() != kNoOffender) return V.flagged(n, flag());
  component_info(run.info, hst, K, has_core ? core_it : 1);
  if (flag() != kNoOffender) return V.flagged(n, flag());
  return sweep_accept(h, V, run.info, hst, rtol, n);
}

// ---- k coupled components: one k x k solve per cell in flow order (sweep.inc: sweep_row_react) -------------------------
// In step_frame with the solve of sweep_step_solve, ascending: per step rhs, the forward levels, the core level iterated
// by block Jacobi, the backward levels, then g and F = rhs - image over all rows and ONE host read of their 2k norms and
// the status word.  The state of the step's start stays in its own buffer until the step is accepted.
pfv_status pfv_transport_advance_react(pfv_ctx* h, const double* q, int k, const double* bc_values,
                                       const double* accumulation, const double* source, const double* mobility,
                                       const double* rate, const double* rate_weight, int n_steps, double rtol,
                                       int maxit, double* c, int32_t* steps_done, pfv_solve_info* last) {
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv::ReactPar par;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    if (h->subface_bc) throw Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the components share one discretization: pfv_upwind_discretize with num_components = 1");
    const std::string bad = pfv::react_check(k, rate, mobility);
    if (!bad.empty()) throw Error(PFV_ERR_ARGUMENT, bad);
    require(bc_values && accumulation && c, "bc_values, accumulation and c are required");
    require(n_steps >= 0, "bad argument");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)(k + 1) * (int64_t)std::max(nc, nf) >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "(k + 1) x cells (faces) beyond int32 indices");
    par = pfv::react_make(k, rate, mobility);
    be_h2d(h->rc_par.ensure(sizeof(par) / sizeof(double)), &par, sizeof(par), h->stream);
    if (q) vec_in(h, h->rc_q.ensure(nf), q, nf);
    vec_in(h, h->rc_bc.ensure(k * nf), bc_values, k * nf);  // component-major, as they came
    vec_in(h, h->rc_acc_in.ensure(k * nc), accumulation, k * nc);
    if (source) vec_in(h, h->rc_src_in.ensure(k * nc), source, k * nc);
    if (rate_weight) vec_in(h, h->rc_rho.ensure(nc), rate_weight, nc);
    vec_in(h, h->rc_c_in.ensure(k * nc), c, k * nc);
    d_q = q ? h->rc_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    int32_t off[pfv::kReactChecks];
    pfv::sweep_react_check_inputs(*h, d_q, k, h->rc_bc.p, h->rc_acc_in.p, rate_weight ? h->rc_rho.p : nullptr,
                                  h->rc_c_in.p, h->rc_par.p, off);
    react_inputs_refused(off, k);
    transport_system(h, S, d_q, h->rc_bc.p, [&] {
      pfv::multi_interleave(*h, (int64_t)nc, k, h->rc_acc_in.p, h->rc_acc.ensure(k * nc));
      if (source) pfv::multi_interleave(*h, (int64_t)nc, k, h->rc_src_in.p, h->rc_src.ensure(k * nc));
      pfv::multi_interleave(*h, (int64_t)nc, k, h->rc_c_in.p, h->rc_x.ensure(k * nc));
      pfv::upwind_bref_react(*h, k, d_q, h->rc_bc.p, h->rc_par.p, h->rc_bref.ensure(k * nc));
      for (pfv::Buf<double>* b : {&h->rc_z, &h->rc_prev, &h->rc_rhs, &h->rc_g, &h->rc_F}) b->ensure(k * nc);
      h->rc_out.ensure(2 * (size_t)k + 1);
    });
  });
  if (st != PFV_OK) return st;

  StepRun run;
  run.info.assign((size_t)k, pfv_solve_info{});
  st = step_frame(h, S, run, n_steps, steps_done, [&](int step) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double* val = cx.val[PFV_MAT_TRANSPORT_SYSTEM].p;
    const double* rho = rate_weight ? cx.rc_rho.p : nullptr;
    double* out = cx.rc_out.p;
    int32_t* status = reinterpret_cast<int32_t*>(out + 2 * k);
    pfv::ReactRow A{cx.pat_T.indptr, cx.pat_T.indices, sw.lev(false), val, cx.diag_t.p, cx.rc_acc.p, rho,
                    cx.rc_rhs.p, nullptr, cx.rc_z.p, status};
    pfv::ReactRow Ac = A;  // the core level, with the state of the previous iterate
    Ac.c_prev = cx.rc_prev.p;
    pfv::upwind_step_rhs_multi(cx, k, cx.rc_acc.p, source ? cx.rc_src.p : nullptr, cx.rc_bref.p, cx.rc_x.p, cx.rc_rhs.p);
    pfv::be_memset(status, 0x7f, sizeof(double), cx.stream);
    SweepSolve V{k, -1, out, kForwardSweep};
    V.levels = [&](int from, int to) { return pfv::sweep_apply_react(cx, sw, from, to, k, A, par); };
    V.core_start = [&] { pfv::sweep_core_copy(cx, sw, k, cx.rc_x.p, cx.rc_z.p); };  // the state of the step's start
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, k, cx.rc_z.p, cx.rc_prev.p);
      pfv::sweep_levels_react(cx, sw, sw.core_level, sw.core_level + 1, k, Ac, par);
    };
    V.norms = [&](bool core_only) {  // from hst: (g_a, g_a), (F_a, F_a)
      pfv::sweep_react_image(cx, cx.pat_T, val, k, cx.rc_acc.p, rho, cx.rc_rhs.p, cx.rc_par.p, cx.rc_z.p, A.lev,
                             core_only ? sw.core_level : -1, cx.rc_g.p, cx.rc_F.p);
      pfv::sweep_react_norms(cx, cx.nc, k, cx.rc_g.p, cx.rc_F.p, out);
    };
    V.flagged = [&](int n, int32_t cell) {
      cx.err = "step " + std::to_string(n) + ": the block of cell " + std::to_string(cell) +
               " has a pivot that is not positive and finite";
      return PFV_ERR_NOT_CONVERGED;
    };
    const pfv_status verdict = sweep_step_solve(h, V, run, rtol, maxit, step);
    if (verdict != PFV_OK) return verdict;
    cx.rc_x.swap(cx.rc_z);
    ++run.completed;
    return PFV_OK;
  }, [&](pfv_status) {
    pfv::multi_deinterleave(*h, (int64_t)nc, k, h->rc_x.p, h->rc_c_in.p);
    vec_out(h, c, h->rc_c_in.p, k * nc);
  });
  if (last)
    for (int a = 0; a < k; ++a) {
      last[a] = run.info[(size_t)a];
      if (run.completed > 0) last[a].solve_ms = run.ms / run.completed;
    }
  h->stats.transport_react_ms = run.ms;
  h->stats.transport_react_steps = run.completed;
  h->stats.transport_react_core_iterations = run.core_total;
  h->stats.transport_react_components = k;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

// ---- sorbing transport: one scalar root per cell and component in flow order (sweep.inc: sweep_row_sorb) ----------------
// In step_frame with the solve of sweep_step_solve, ascending: per step rhs, the forward levels, the core level iterated
// by nonlinear Jacobi, the backward levels, then the image and its 2k norms over all rows and ONE host read of them and
// the flag word.  The state of the step's start and its sigma = S(c) stay in their own buffers until the step is accepted.
static void sorb_inputs_refused(const int32_t (&off)[pfv::kSorbChecks], int k) {
  static const char* const what[pfv::kSorbChecks] = {
      "accumulation must be positive: cell ", "capacity must not be negative: cell ",
      "c must be non-negative and finite: cell ", "Dirichlet inflow value must be non-negative and finite: face ",
      "Neumann value is not finite on face ", pfv::kUnmarkedInflowFace};
  inputs_refused(off, pfv::kSorbChecks, what, 0x1fu, k, 0);
}

pfv_status pfv_transport_advance_sorb(pfv_ctx* h, const double* q, int k, const int32_t* isotherm_kind,
                                      const double* isotherm_params, const double* bc_values,
                                      const double* accumulation, const double* capacity, const double* source,
                                      int n_steps, double rtol, int maxit, double* c, double* sorbed_out,
                                      int32_t* steps_done, pfv_solve_info* last) {
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  std::vector<pfv::Isotherm> iso;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    if (h->subface_bc) throw Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the components share one discretization: pfv_upwind_discretize with num_components = 1");
    if (k < 1 || k > 64) throw Error(PFV_ERR_ARGUMENT, "k must lie in 1 .. 64 (k = " + std::to_string(k) + ")");
    require(isotherm_kind && isotherm_params, "isotherm_kind and isotherm_params are required");
    iso.resize((size_t)k);
    for (int a = 0; a < k; ++a) {
      const double p0 = isotherm_params[2 * a], p1 = isotherm_params[2 * a + 1];
      const std::string bad = pfv::isotherm_check(isotherm_kind[a], p0, p1);
      if (!bad.empty()) throw Error(PFV_ERR_ARGUMENT, "isotherm of component " + std::to_string(a) + ": " + bad);
      iso[(size_t)a] = pfv::isotherm_make(isotherm_kind[a], p0, p1);
    }
    require(bc_values && accumulation && c, "bc_values, accumulation and c are required");
    require(n_steps >= 0, "bad argument");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)(k + 1) * (int64_t)std::max(nc, nf) >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "(k + 1) x cells (faces) beyond int32 indices");
    be_h2d(h->sb_par.ensure(3 * (size_t)k), iso.data(), sizeof(pfv::Isotherm) * (size_t)k, h->stream);
    if (q) vec_in(h, h->sb_q.ensure(nf), q, nf);
    vec_in(h, h->sb_bc.ensure(k * nf), bc_values, k * nf);  // component-major, as they came
    vec_in(h, h->sb_acc_in.ensure(k * nc), accumulation, k * nc);
    if (capacity) vec_in(h, h->sb_cap_in.ensure(k * nc), capacity, k * nc);
    if (source) vec_in(h, h->sb_src_in.ensure(k * nc), source, k * nc);
    vec_in(h, h->sb_c_in.ensure(k * nc), c, k * nc);
    d_q = q ? h->sb_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    int32_t off[pfv::kSorbChecks];
    pfv::sweep_sorb_check_inputs(*h, d_q, k, h->sb_bc.p, h->sb_acc_in.p, capacity ? h->sb_cap_in.p : nullptr,
                                 h->sb_c_in.p, off);
    sorb_inputs_refused(off, k);
    transport_system(h, S, d_q, h->sb_bc.p, [&] {
      pfv::multi_interleave(*h, (int64_t)nc, k, h->sb_acc_in.p, h->sb_acc.ensure(k * nc));
      if (capacity) pfv::multi_interleave(*h, (int64_t)nc, k, h->sb_cap_in.p, h->sb_cap.ensure(k * nc));
      if (source) pfv::multi_interleave(*h, (int64_t)nc, k, h->sb_src_in.p, h->sb_src.ensure(k * nc));
      pfv::multi_interleave(*h, (int64_t)nc, k, h->sb_c_in.p, h->sb_x.ensure(k * nc));
      pfv::upwind_bref_multi(*h, k, d_q, h->sb_bc.p, h->sb_bref.ensure(k * nc));
      for (pfv::Buf<double>* b : {&h->sb_accf, &h->sb_capn, &h->sb_sx, &h->sb_z, &h->sb_sz, &h->sb_prev, &h->sb_rhs})
        b->ensure(k * nc);
      h->sb_out.ensure(2 * (size_t)k + 1);
      pfv::sweep_sorb_setup(*h, k, reinterpret_cast<const pfv::Isotherm*>(h->sb_par.p), h->sb_acc.p,
                            capacity ? h->sb_cap.p : nullptr, h->sb_x.p, h->sb_accf.p, h->sb_capn.p, h->sb_sx.p);
    });
  });
  if (st != PFV_OK) return st;

  StepRun run;
  run.info.assign((size_t)k, pfv_solve_info{});
  st = step_frame(h, S, run, n_steps, steps_done, [&](int step) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double* val = cx.val[PFV_MAT_TRANSPORT_SYSTEM].p;
    const double* capn = capacity ? cx.sb_capn.p : nullptr;
    double* out = cx.sb_out.p;
    int32_t* status = reinterpret_cast<int32_t*>(out + 2 * k);
    pfv::SorbRow A{cx.pat_T.indptr, cx.pat_T.indices, sw.lev(false), val, cx.diag_t.p, cx.sb_accf.p, capn, cx.sb_rhs.p,
                   reinterpret_cast<const pfv::Isotherm*>(cx.sb_par.p), cx.sb_x.p, nullptr, cx.sb_z.p, cx.sb_sz.p, status};
    pfv::SorbRow Ac = A;  // the core level: the previous iterate for the in-core neighbours and as the start value
    Ac.c_prev = Ac.c_start = cx.sb_prev.p;
    pfv::upwind_step_rhs_sorb(cx, k, cx.sb_accf.p, capn, source ? cx.sb_src.p : nullptr, cx.sb_bref.p, cx.sb_x.p,
                              cx.sb_sx.p, cx.sb_rhs.p);
    pfv::be_memset(status, 0x7f, sizeof(double), cx.stream);
    SweepSolve V{k, -1, out, kForwardSweep};
    V.levels = [&](int from, int to) { return pfv::sweep_apply_sorb(cx, sw, from, to, k, A); };
    V.core_start = [&] { pfv::sweep_core_copy(cx, sw, k, cx.sb_x.p, cx.sb_z.p); };  // the state of the step's start
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, k, cx.sb_z.p, cx.sb_prev.p);
      pfv::sweep_levels_sorb(cx, sw, sw.core_level, sw.core_level + 1, k, Ac);
    };
    V.norms = [&](bool core_only) {  // from hst: (rhs_a, rhs_a), (F_a, F_a)
      pfv::sweep_sorb_norms(cx, cx.pat_T, val, k, cx.sb_accf.p, capn, cx.sb_rhs.p, cx.sb_z.p, cx.sb_sz.p, A.lev,
                            core_only ? sw.core_level : -1, out);
    };
    V.flag_ends_core = true;  // (a row without a root c >= 0: the input admits no solution)
    V.flagged = [&](int n, int32_t at) -> pfv_status {
      throw Error(PFV_ERR_ARGUMENT, "step " + std::to_string(n) + " leaves c >= 0: no root in cell " +
                                        std::to_string(at / k) + ", component " + std::to_string(at % k));
    };
    const pfv_status verdict = sweep_step_solve(h, V, run, rtol, maxit, step);
    if (verdict != PFV_OK) return verdict;
    cx.sb_x.swap(cx.sb_z);
    cx.sb_sx.swap(cx.sb_sz);
    ++run.completed;
    return PFV_OK;
  }, [&](pfv_status) {
    pfv::multi_deinterleave(*h, (int64_t)nc, k, h->sb_x.p, h->sb_c_in.p);
    vec_out(h, c, h->sb_c_in.p, k * nc);
    if (sorbed_out) {
      pfv::multi_deinterleave(*h, (int64_t)nc, k, h->sb_sx.p, h->sb_c_in.p);
      vec_out(h, sorbed_out, h->sb_c_in.p, k * nc);
    }
  });
  if (last)
    for (int a = 0; a < k; ++a) {
      last[a] = run.info[(size_t)a];
      if (run.completed > 0) last[a].solve_ms = run.ms / run.completed;
    }
  h->stats.transport_sorb_ms = run.ms;
  h->stats.transport_sorb_steps = run.completed;
  h->stats.transport_sorb_core_iterations = run.core_total;
  h->stats.transport_sorb_components = k;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

// ---- the observation of an adjoint call, shared by pfv_transport_adjoint_multi and pfv_transport_adjoint_react --------
// obs_cells (host) are checked, the loads [N][k][n_obs] go to aj_loads and are checked for finiteness
static void adjoint_take_loads(pfv_ctx* h, int k, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                               const double* loads) {
  const size_t nc = (size_t)h->nc;
  if (obs_cells) {
    require(n_obs >= 0 && n_obs <= (int64_t)nc, "n_obs must lie in 0 .. the number of cells");
    std::vector<char> seen(nc, 0);
    for (int64_t m = 0; m < n_obs; ++m) {
      const int32_t cell = obs_cells[m];
      if (cell < 0 || (size_t)cell >= nc)
        throw Error(PFV_ERR_ARGUMENT, "obs_cells[" + std::to_string(m) + "] = " + std::to_string(cell) +
                                          " is out of range (0 .. " + std::to_string(nc - 1) + ")");
      if (seen[(size_t)cell])
        throw Error(PFV_ERR_ARGUMENT, "obs_cells[" + std::to_string(m) + "] = " + std::to_string(cell) + " is repeated");
      seen[(size_t)cell] = 1;
    }
  } else {
    require(n_obs == (int64_t)nc, "obs_cells == NULL means every cell: n_obs must be the number of cells");
  }
  const size_t nl = (size_t)n_steps * k * (size_t)n_obs;
  if (nl) {
    vec_in(h, h->aj_loads.ensure(nl), loads, nl);
    const int64_t bad = nl < (size_t(1) << 31) ? pfv::adjoint_first_nonfinite(*h, (int64_t)nl, h->aj_loads.p) : -1;
    if (bad >= 0) {
      const int64_t per = (int64_t)k * n_obs;
      throw Error(PFV_ERR_ARGUMENT, "loads is not finite at step " + std::to_string(bad / per + 1) + ", component " +
                                        std::to_string(bad % per / n_obs) + ", observation " +
                                        std::to_string(bad % n_obs));
    }
  }
}

// aj_slot: the position of every cell among the observation cells (after adjoint_take_loads; nothing for obs_cells == NULL)
static void adjoint_take_slots(pfv_ctx* h, int64_t n_obs, const int32_t* obs_cells) {
  const size_t nc = (size_t)h->nc;
  if (obs_cells && n_obs > 0) {
    be_h2d(h->aj_obs.ensure((size_t)n_obs), obs_cells, sizeof(int32_t) * (size_t)n_obs, h->stream);
    pfv::be_memset(h->aj_slot.ensure(nc), 0xff, sizeof(int32_t) * nc, h->stream);
    pfv::adjoint_obs_slots(*h, n_obs, h->aj_obs.p, h->aj_slot.p);
  } else if (obs_cells) {
    pfv::be_memset(h->aj_slot.ensure(nc), 0xff, sizeof(int32_t) * nc, h->stream);
  }
}

// ---- the set-up the four adjoint calls share ---------------------------------------------------------------------------
// the counts of a call; loads: whether the observation has its loads
static void adjoint_check_counts(int n_steps, double rtol, int maxit, bool loads,
                                 const char* loads_text = "loads is required") {
  require(n_steps >= 0, "bad argument");
  require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
  require(loads || n_steps == 0, loads_text);
}

// The system of an adjoint call: transport_system, where what the call does on A's rows (own_rows) is followed by A's
// transposed values and the observation's slots; the flow order comes last.
static void adjoint_system(pfv_ctx* h, StepSetup& S, const double* d_q, const double* d_bc, int64_t n_obs,
                           const int32_t* obs_cells, const std::function<void()>& own_rows = nullptr) {
  transport_system(h, S, d_q, d_bc, [&] {
    if (own_rows) own_rows();
    const size_t nnz = (size_t)std::max<int64_t>(h->pat_T.nnz, 1);
    if (!h->have_tpos_T) {
      pfv::sweep_transpose_positions(*h, h->pat_T, h->tpos_T.ensure(nnz));
      h->have_tpos_T = true;
    }
    pfv::sweep_transpose_values(*h, h->pat_T.nnz, h->tpos_T.p, h->val[PFV_MAT_TRANSPORT_SYSTEM].p, h->valT_T.ensure(nnz));
    adjoint_take_slots(h, n_obs, obs_cells);
  });
}

// the two slabs of the states [k][nc] a step reads, and where a slab in host memory lands
static void adjoint_slab_buffers(pfv_ctx* h, int k) {
  const size_t n = (size_t)k * (size_t)h->nc;
  h->aj_sA.ensure(n);
  h->aj_sB.ensure(n);
  if (!h->vectors_on_device) h->aj_state_in.ensure(n);
}

// ---- the steps of the adjoint calls, in step_frame (after their set-up, with the timer running) --------------------------
// Per step n = N .. 1: one slab of states (stage), the right-hand side fused with what the multipliers of step n + 1 add
// to the cell gradients (rhs), the call's own solve -- sweep, core, acceptance --, its gradients of the accepted step,
// the swap of the multipliers and the slabs.  After the last step the right-hand-side pass runs once more without loads
// (rhs with n = 0): what it leaves is the gradient with respect to the start.  Then the gradients go out, and the
// transport system is dropped.
enum class GradLayout { plain, by_cell, host };  // by_cell: [cell][k] on the device, [k][cell] for the caller
struct AdjointGrad {  // one output of a call
  double* to;             // the caller's array; nullptr: not wanted
  pfv::Buf<double>* buf;  // where it is summed on the device
  size_t n;               // elements
  GradLayout layout;      // host: `to` is host memory whatever the handle's vectors are (as its parameters are)
  bool summed = true;     // over the steps, from zero; false: what the last right-hand-side pass leaves in buf
};
struct AdjointCall {  // what the calls share, by the callers' names
  int k, n_steps;
  int64_t n_obs;
  const int32_t* obs_cells;
  // what the default hooks read: the states [N + 1][k][nc] or nullptr, the accumulation on the device, interleaved,
  // and whether these two gradients are wanted
  const double* states;
  const double* acc;
  const double *grad_source, *grad_accumulation;
  int32_t* steps_done;
  pfv_solve_info* last;
  std::vector<AdjointGrad> grads;
  int saturation = -1;  // the index of the saturation's norms behind the k components' (reported first), or none
  // The hooks; the defaults are those of one multiplier per component: lambda in aj_lam / aj_lam2, the slabs in aj_sA /
  // aj_sB.
  std::function<void(int)> stage;      // slab n into the buffers of the step at hand (n = 0: for the last pass)
  std::function<void(int, bool)> rhs;  // the right-hand side(s) of step n, or of the last pass; whether step n + 1 ran
  std::function<void()> swap;          // the accepted step becomes step n + 1
};
// solve(n, z) -> PFV_OK or the verdict of a refused step (its text in h->err): the multipliers of step n, lambda^n into
// z, from the right-hand side(s); it fills run.info and counts run.launches / run.core_total (sweep_step_solve).
// step_grads(z): what the accepted step adds to the gradients the right-hand-side pass does not sum.
static pfv_status adjoint_steps(pfv_ctx* h, StepSetup& S, const AdjointCall& A, StepRun& run,
                                const std::function<pfv_status(int, double*)>& solve,
                                const std::function<void(double*)>& step_grads) {
  pfv::pfv_ctx_impl& cx = *h;
  const int k = A.k;
  const size_t nc = (size_t)h->nc;
  const auto stage = A.stage ? A.stage : [&](int n) {  // (c^0 only where the last pass reads it)
    if (!A.states || (n == 0 && !A.grad_accumulation)) return;
    const double* src = A.states + (size_t)n * k * nc;
    if (!h->vectors_on_device) {
      be_h2d(cx.aj_state_in.p, src, sizeof(double) * k * nc, cx.stream);
      src = cx.aj_state_in.p;
    }
    pfv::multi_interleave(cx, (int64_t)nc, k, src, cx.aj_sB.p);  // c^n; aj_sA holds c^{n+1}
  };
  // g^n + acc o lambda^{n+1}, fused with what lambda^{n+1} adds to grad_source and grad_accumulation (adjoint_step_rhs);
  // the last pass leaves acc o lambda^1
  const auto rhs = A.rhs ? A.rhs : [&](int n, bool have_next) {
    if (n == 0 && !have_next) {
      pfv::be_memset(cx.aj_r.p, 0, sizeof(double) * k * nc, cx.stream);
      return;
    }
    pfv::adjoint_step_rhs(cx, k, A.acc, have_next ? cx.aj_lam.p : nullptr, n > 0 && A.obs_cells ? cx.aj_slot.p : nullptr,
                          n > 0 ? cx.aj_loads.p + (size_t)(n - 1) * k * (size_t)A.n_obs : nullptr, n > 0 ? A.n_obs : 0,
                          cx.aj_sB.p, cx.aj_sA.p, A.grad_source ? cx.aj_gsrc.p : nullptr,
                          A.grad_accumulation ? cx.aj_gacc.p : nullptr, cx.aj_r.p);
  };
  const auto swap = A.swap ? A.swap : [&] {
    cx.aj_lam.swap(cx.aj_lam2);
    cx.aj_sA.swap(cx.aj_sB);
  };
  run.info.assign((size_t)k + (A.saturation >= 0 ? 1 : 0), pfv_solve_info{});
  bool have_next = false;  // the multipliers of step n + 1 are there
  // (the frame counts upwards: its step is N - n, and the last pass, n = 0, is one more step that completes none)
  const pfv_status st = step_frame(h, S, run, A.n_steps + 1, A.steps_done, [&](int step) -> pfv_status {
    const int n = A.n_steps - step;
    if (step == 0)
      for (const AdjointGrad& g : A.grads)
        if (g.to && g.summed) pfv::be_memset(g.buf->ensure(g.n), 0, sizeof(double) * g.n, cx.stream);
    if (n == 0) {
      if (have_next) stage(0);
      rhs(0, have_next);
      return PFV_OK;
    }
    stage(n);
    rhs(n, have_next);
    double* z = cx.aj_lam2.p;
    const pfv_status verdict = solve(n, z);
    if (verdict != PFV_OK) return verdict;
    step_grads(z);
    swap();
    have_next = true;
    ++run.completed;
    return PFV_OK;
  }, [&](pfv_status ended) {  // a call that failed or was refused hands no gradient out
    if (ended != PFV_OK) return;
    for (const AdjointGrad& g : A.grads) {
      if (!g.to) continue;
      if (g.layout == GradLayout::host) {
        be_d2h(g.to, g.buf->p, sizeof(double) * g.n, cx.stream);
      } else if (g.layout == GradLayout::by_cell) {
        pfv::multi_deinterleave(cx, (int64_t)nc, k, g.buf->p, cx.mc_c.p);
        vec_out(h, g.to, cx.mc_c.p, g.n);
      } else {
        vec_out(h, g.to, g.buf->p, g.n);
      }
    }
  });
  if (A.last) {
    int to = 0;
    if (A.saturation >= 0) A.last[to++] = run.info[(size_t)A.saturation];
    for (int a = 0; a < (int)run.info.size(); ++a)
      if (a != A.saturation) A.last[to++] = run.info[(size_t)a];
    if (run.completed > 0)
      for (int a = 0; a < to; ++a) A.last[a].solve_ms = run.ms / run.completed;
  }
  return st;
}

// ---- the adjoint of the k-component step: one transposed sweep in reverse flow order per step (sweep.inc) -------------
// In the frame of adjoint_steps with the solve of sweep_step_solve on the rows of sweep_row_multi_t; after an accepted
// step the two face kernels (grad_bc_values, grad_flux).
pfv_status pfv_transport_adjoint_multi(pfv_ctx* h, const double* q, int n_comp, const double* bc_values,
                                       const double* accumulation, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                       const double* loads, const double* states, double rtol, int maxit,
                                       double* grad_c0, double* grad_source, double* grad_bc_values,
                                       double* grad_accumulation, double* grad_flux, int32_t* steps_done,
                                       pfv_solve_info* last) {
  const int k = n_comp;
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the components share one discretization: pfv_upwind_discretize with num_components = 1");
    require(n_comp >= 1 && n_comp <= 64, "n_comp must lie in 1 .. 64");
    require(bc_values && accumulation, "bc_values and accumulation are required");
    adjoint_check_counts(n_steps, rtol, maxit, loads != nullptr);
    require(states || !grad_accumulation, "grad_accumulation needs states (c^0 .. c^N)");
    require(states || !grad_flux, "grad_flux needs states (c^0 .. c^N)");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)nc * k >= (int64_t(1) << 31) || (int64_t)nf * k >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "n_comp x cells (faces) beyond int32 indices");
    adjoint_take_loads(h, k, n_steps, n_obs, obs_cells, loads);
    if (q) vec_in(h, h->mc_q.ensure(nf), q, nf);
    vec_in(h, h->mc_bc.ensure(k * nf), bc_values, k * nf);
    vec_in(h, h->mc_acc.ensure(k * nc), accumulation, k * nc);
    d_q = q ? h->mc_q.p : h->upw_q.p;
    adjoint_system(h, S, d_q, h->mc_bc.p, n_obs, obs_cells, [&] {
      pfv::multi_interleave(*h, (int64_t)nc, k, h->mc_acc.p, h->mc_acc_i.ensure(k * nc));
      const int64_t zd = pfv::upwind_zero_diag_multi(*h, k, h->diag_t.p, h->mc_acc_i.p);
      if (zd >= 0) throw Error(PFV_ERR_UNSUPPORTED, zero_diagonal_text(zd, k));
    });
    for (pfv::Buf<double>* b : {&h->aj_lam, &h->aj_lam2, &h->aj_prev, &h->aj_r, &h->mc_c}) b->ensure(k * nc);
    if (states) adjoint_slab_buffers(h, k);
    h->mc_nrm.ensure(2 * (size_t)k);
  });
  if (st != PFV_OK) return st;

  StepRun run;
  AdjointCall call{k, n_steps, n_obs, obs_cells, states, h->mc_acc_i.p, grad_source, grad_accumulation, steps_done,
                   last};
  call.grads = {{grad_c0, &h->aj_r, k * nc, GradLayout::by_cell, false},
                {grad_source, &h->aj_gsrc, k * nc, GradLayout::by_cell},
                {grad_accumulation, &h->aj_gacc, k * nc, GradLayout::by_cell},
                {grad_bc_values, &h->aj_gbc, k * nf, GradLayout::plain},
                {grad_flux, &h->aj_gq, nf, GradLayout::plain}};
  st = adjoint_steps(h, S, call, run, [&](int n, double* z) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double *valT = cx.valT_T.p, *acc = cx.mc_acc_i.p;
    SweepSolve V{k, -1, cx.mc_nrm.p, kAdjointSweep};
    V.levels = [&](int from, int to) {
      return pfv::sweep_apply_multi_t(cx, sw, from, to, cx.pat_T, valT, cx.diag_t.p, acc, k, cx.aj_r.p, z);
    };
    V.core_start = [&] { pfv::sweep_core_zero(cx, sw, k, z); };
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, k, z, cx.aj_prev.p);
      pfv::sweep_core_multi_t(cx, sw, cx.pat_T, valT, cx.diag_t.p, acc, k, cx.aj_r.p, cx.aj_prev.p, z);
    };
    V.norms = [&](bool core_only) {  // (valT: the image under S^T)
      if (core_only) pfv::sweep_core_norms_multi_t(cx, sw, cx.pat_T, valT, acc, k, cx.aj_r.p, z, cx.mc_nrm.p);
      else pfv::sweep_residual_norms_multi(cx, cx.pat_T, valT, acc, k, cx.aj_r.p, z, cx.mc_nrm.p);
    };
    return sweep_step_solve(h, V, run, rtol, maxit, n);
  }, [&](double* z) {
    if (grad_bc_values) pfv::adjoint_grad_bc(*h, k, d_q, z, h->aj_gbc.p);
    if (grad_flux) pfv::adjoint_grad_flux(*h, k, h->mc_bc.p, z, h->aj_sB.p, h->aj_gq.p);
  });
  h->stats.transport_adjoint_ms = run.ms;
  h->stats.transport_adjoint_steps = run.completed;
  h->stats.transport_adjoint_core_iterations = run.core_total;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

// ---- the adjoint of the reactive step: one transposed k x k sweep in reverse flow order per step (sweep.inc) ----------
// The frame and the solve are those of pfv_transport_adjoint_multi with the row, the norms and the core of
// pfv_transport_advance_react in the transposed system M^T lambda^n = g^n + acc o lambda^{n+1}: the rows read valT and a
// ReactPar that holds K^T (sweep_row_react<K, Descending>), the image and the scale g~_a = r_a - rho sum_{b != a} K_ba
// lambda_b come from sweep_react_image on the same two.  After an accepted step the face kernels take the mobility and
// the two rate gradients are added in step order (adjoint_grad_rate, adjoint_grad_rate_weight).
pfv_status pfv_transport_adjoint_react(pfv_ctx* h, const double* q, int k, const double* bc_values,
                                       const double* accumulation, const double* mobility, const double* rate,
                                       const double* rate_weight, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                       const double* loads, const double* states, double rtol, int maxit,
                                       double* grad_c0, double* grad_source, double* grad_bc_values,
                                       double* grad_accumulation, double* grad_flux, double* grad_rate,
                                       double* grad_rate_weight, int32_t* steps_done, pfv_solve_info* last) {
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv::ReactPar par, parT;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    upwind_supported(h);
    if (h->subface_bc) throw Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
    require(h->have_upwind, "pfv_upwind_discretize first");
    require(h->upw_ncomp == 1, "the components share one discretization: pfv_upwind_discretize with num_components = 1");
    const std::string bad = pfv::react_check(k, rate, mobility);  // (the caller's K, not its transpose)
    if (!bad.empty()) throw Error(PFV_ERR_ARGUMENT, bad);
    require(bc_values && accumulation, "bc_values and accumulation are required");
    adjoint_check_counts(n_steps, rtol, maxit, loads != nullptr);
    require(states || !grad_accumulation, "grad_accumulation needs states (c^0 .. c^N)");
    require(states || !grad_flux, "grad_flux needs states (c^0 .. c^N)");
    require(states || !grad_rate, "grad_rate needs states (c^0 .. c^N)");
    require(states || !grad_rate_weight, "grad_rate_weight needs states (c^0 .. c^N)");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)(k + 1) * (int64_t)std::max(nc, nf) >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "(k + 1) x cells (faces) beyond int32 indices");
    par = pfv::react_make(k, rate, mobility);
    parT = par;
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b) parT.K[a * k + b] = par.K[b * k + a];
    be_h2d(h->rc_par.ensure(sizeof(par) / sizeof(double)), &par, sizeof(par), h->stream);
    be_h2d(h->rc_parT.ensure(sizeof(parT) / sizeof(double)), &parT, sizeof(parT), h->stream);
    adjoint_take_loads(h, k, n_steps, n_obs, obs_cells, loads);
    if (q) vec_in(h, h->rc_q.ensure(nf), q, nf);
    vec_in(h, h->rc_bc.ensure(k * nf), bc_values, k * nf);  // component-major, as they came
    vec_in(h, h->rc_acc_in.ensure(k * nc), accumulation, k * nc);
    if (rate_weight) vec_in(h, h->rc_rho.ensure(nc), rate_weight, nc);
    d_q = q ? h->rc_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    int32_t off[pfv::kReactChecks];  // (the call has no state to check: the accumulation stands in)
    pfv::sweep_react_check_inputs(*h, d_q, k, h->rc_bc.p, h->rc_acc_in.p, rate_weight ? h->rc_rho.p : nullptr,
                                  h->rc_acc_in.p, h->rc_par.p, off);
    react_inputs_refused(off, k, kReactState);
    adjoint_system(h, S, d_q, h->rc_bc.p, n_obs, obs_cells, [&] {
      pfv::multi_interleave(*h, (int64_t)nc, k, h->rc_acc_in.p, h->rc_acc.ensure(k * nc));
    });
    for (pfv::Buf<double>* b : {&h->aj_lam, &h->aj_lam2, &h->aj_r, &h->rc_prev, &h->rc_g, &h->rc_F, &h->mc_c})
      b->ensure(k * nc);
    if (states) adjoint_slab_buffers(h, k);
    h->rc_out.ensure(2 * (size_t)k + 1);
  });
  if (st != PFV_OK) return st;

  StepRun run;
  const double* rho = rate_weight ? h->rc_rho.p : nullptr;
  AdjointCall call{k, n_steps, n_obs, obs_cells, states, h->rc_acc.p, grad_source, grad_accumulation, steps_done, last};
  call.grads = {{grad_c0, &h->aj_r, k * nc, GradLayout::by_cell, false},
                {grad_source, &h->aj_gsrc, k * nc, GradLayout::by_cell},
                {grad_accumulation, &h->aj_gacc, k * nc, GradLayout::by_cell},
                {grad_bc_values, &h->aj_gbc, k * nf, GradLayout::plain},
                {grad_flux, &h->aj_gq, nf, GradLayout::plain},
                {grad_rate_weight, &h->aj_grho, nc, GradLayout::plain},
                {grad_rate, &h->aj_gK, (size_t)k * k, GradLayout::host}};
  st = adjoint_steps(h, S, call, run, [&](int n, double* z) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double *valT = cx.valT_T.p, *acc = cx.rc_acc.p;
    double* out = cx.rc_out.p;
    int32_t* status = reinterpret_cast<int32_t*>(out + 2 * k);
    pfv::ReactRow A{cx.pat_T.indptr, cx.pat_T.indices, sw.lev(false), valT, cx.diag_t.p, acc, rho,
                    cx.aj_r.p, nullptr, z, status};
    pfv::ReactRow Ac = A;  // the core level, with the previous iterate
    Ac.c_prev = cx.rc_prev.p;
    pfv::be_memset(status, 0x7f, sizeof(double), cx.stream);
    SweepSolve V{k, -1, out, kAdjointSweep};
    V.levels = [&](int from, int to) {
      return pfv::sweep_apply_react(cx, sw, from, to, k, A, parT, pfv::Descending{});
    };
    V.core_start = [&] { pfv::sweep_core_zero(cx, sw, k, z); };
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, k, z, cx.rc_prev.p);
      pfv::sweep_levels_react(cx, sw, sw.core_level, sw.core_level + 1, k, Ac, parT, pfv::Descending{});
    };
    V.norms = [&](bool core_only) {  // from hst: (g~_a, g~_a), (F_a, F_a)
      pfv::sweep_react_image(cx, cx.pat_T, valT, k, acc, rho, cx.aj_r.p, cx.rc_parT.p, z, A.lev,
                             core_only ? sw.core_level : -1, cx.rc_g.p, cx.rc_F.p, true);
      pfv::sweep_react_norms(cx, cx.nc, k, cx.rc_g.p, cx.rc_F.p, out);
    };
    V.flagged = [&](int step, int32_t cell) {
      cx.err = "adjoint step " + std::to_string(step) + ": the block of cell " + std::to_string(cell) +
               " has a pivot that is not positive and finite";
      return PFV_ERR_NOT_CONVERGED;
    };
    return sweep_step_solve(h, V, run, rtol, maxit, n);
  }, [&](double* z) {
    pfv::pfv_ctx_impl& cx = *h;
    if (grad_bc_values) pfv::adjoint_grad_bc(cx, k, d_q, z, cx.aj_gbc.p, cx.rc_par.p);
    if (grad_flux) pfv::adjoint_grad_flux(cx, k, cx.rc_bc.p, z, cx.aj_sB.p, cx.aj_gq.p, cx.rc_par.p);
    if (grad_rate) pfv::adjoint_grad_rate(cx, k, rho, z, cx.aj_sB.p, cx.aj_gK.p);
    if (grad_rate_weight)
      pfv::adjoint_grad_rate_weight(cx, k, cx.rc_par.p + pfv::kReactMax, z, cx.aj_sB.p, cx.aj_grho.p);
  });
  h->stats.transport_react_adjoint_ms = run.ms;
  h->stats.transport_react_adjoint_steps = run.completed;
  h->stats.transport_react_adjoint_core_iterations = run.core_total;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

// what the two saturation adjoints check before any array is read
static void adjoint_nl_supported(pfv_ctx* h, int fluxfn_kind, const double* fluxfn_params, int n_params,
                                 const double* grad_fluxfn, const double* bc_values, const double* accumulation) {
  upwind_supported(h);
  if (h->subface_bc) throw Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
  require(h->have_upwind, "pfv_upwind_discretize first");
  require(h->upw_ncomp == 1, "the saturation step needs pfv_upwind_discretize with num_components = 1");
  const std::string bad = pfv::fluxfn_check(fluxfn_kind, fluxfn_params, n_params);
  if (!bad.empty()) throw Error(PFV_ERR_ARGUMENT, bad);
  require(!grad_fluxfn || fluxfn_kind == PFV_FLUXFN_COREY,
          "grad_fluxfn is the gradient with respect to the six Corey parameters: PFV_FLUXFN_COREY only");
  require(bc_values && accumulation, "bc_values and accumulation are required");
}

// ---- the adjoint of the saturation step: one transposed sweep on the step's slopes per step (sweep.inc) ---------------
// In the frame of adjoint_steps with k = 1.  The solve of step n: d = f'(s^n) and phi = f(s^n) from the slab the frame
// has staged (one streaming pass), then sweep_step_solve on the rows of J^T = diag(acc) + diag(d) M^T
// (sweep_row_nl_t).  After an accepted step the two face kernels, the sink's cell kernel and the six Corey sums, which
// are added in step order.
pfv_status pfv_transport_adjoint_nl(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                    int n_params, const double* bc_values, const double* accumulation,
                                    const double* sink, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                    const double* loads, const double* states, double rtol, int maxit, double* grad_s0,
                                    double* grad_source, double* grad_bc_values, double* grad_accumulation,
                                    double* grad_sink, double* grad_flux, double* grad_fluxfn, int32_t* steps_done,
                                    pfv_solve_info* last) {
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv::FluxFn F;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    adjoint_nl_supported(h, fluxfn_kind, fluxfn_params, n_params, grad_fluxfn, bc_values, accumulation);
    adjoint_check_counts(n_steps, rtol, maxit, loads != nullptr);
    require(states != nullptr || n_steps == 0, "states (s^0 .. s^N) is required: the step is linearised about them");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    adjoint_take_loads(h, 1, n_steps, n_obs, obs_cells, loads);
    if (q) vec_in(h, h->nl_q.ensure(nf), q, nf);
    vec_in(h, h->nl_bc.ensure(nf), bc_values, nf);
    vec_in(h, h->nl_acc.ensure(nc), accumulation, nc);
    if (sink) vec_in(h, h->nl_sink.ensure(nc), sink, nc);
    d_q = q ? h->nl_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    int32_t off[pfv::kNlChecks];  // (the states are not checked: the accumulation stands in)
    pfv::sweep_nl_check_inputs(*h, d_q, h->nl_bc.p, h->nl_acc.p, sink ? h->nl_sink.p : nullptr, h->nl_acc.p, 0, nullptr,
                               nullptr, nullptr, off);
    nl_inputs_refused(off, 0, kNlStates);
    if (fluxfn_kind == PFV_FLUXFN_TABLE)
      be_h2d(h->nl_table.ensure((size_t)n_params), fluxfn_params, sizeof(double) * (size_t)n_params, h->stream);
    F = pfv::fluxfn_make(fluxfn_kind, fluxfn_params, n_params, h->nl_table.p);
    adjoint_system(h, S, d_q, h->nl_bc.p, n_obs, obs_cells);
    for (pfv::Buf<double>* b : {&h->aj_lam, &h->aj_lam2, &h->aj_prev, &h->aj_r, &h->aj_d, &h->aj_phi, &h->mc_c})
      b->ensure(nc);
    adjoint_slab_buffers(h, 1);
    h->mc_nrm.ensure(2);
  });
  if (st != PFV_OK) return st;

  StepRun run;
  const double* d_sink = sink ? h->nl_sink.p : nullptr;
  AdjointCall call{1, n_steps, n_obs, obs_cells, states, h->nl_acc.p, grad_source, grad_accumulation, steps_done, last};
  call.grads = {{grad_s0, &h->aj_r, nc, GradLayout::by_cell, false},
                {grad_source, &h->aj_gsrc, nc, GradLayout::by_cell},
                {grad_accumulation, &h->aj_gacc, nc, GradLayout::by_cell},
                {grad_bc_values, &h->aj_gbc, nf, GradLayout::plain},
                {grad_flux, &h->aj_gq, nf, GradLayout::plain},
                {grad_sink, &h->aj_gsink, nc, GradLayout::plain},
                {grad_fluxfn, &h->aj_gF, 6, GradLayout::host}};
  st = adjoint_steps(h, S, call, run, [&](int n, double* z) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double *valT = cx.valT_T.p, *acc = cx.nl_acc.p, *d = cx.aj_d.p, *diag = cx.diag_t.p;
    pfv::adjoint_nl_slopes(cx, F, cx.aj_sB.p, cx.aj_d.p, cx.aj_phi.p);  // of s^n
    SweepSolve V{1, -1, cx.mc_nrm.p, kAdjointSweep};
    V.levels = [&](int from, int to) {
      return pfv::sweep_apply_nl_t(cx, sw, from, to, cx.pat_T, valT, diag, d_sink, acc, d, cx.aj_r.p, z);
    };
    V.core_start = [&] { pfv::sweep_core_zero(cx, sw, 1, z); };
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, 1, z, cx.aj_prev.p);
      pfv::sweep_core_nl_t(cx, sw, cx.pat_T, valT, diag, d_sink, acc, d, cx.aj_r.p, cx.aj_prev.p, z);
    };
    V.norms = [&](bool core_only) {
      pfv::sweep_norms_nl_t(cx, sw, cx.pat_T, valT, d_sink, acc, d, cx.aj_r.p, z, core_only, cx.mc_nrm.p);
    };
    return sweep_step_solve(h, V, run, rtol, maxit, n);
  }, [&](double* z) {
    pfv::pfv_ctx_impl& cx = *h;
    if (grad_sink) pfv::adjoint_nl_grad_sink(cx, z, cx.aj_phi.p, cx.aj_gsink.p);
    if (grad_bc_values) pfv::adjoint_nl_grad_bc(cx, F, d_q, cx.nl_bc.p, z, cx.aj_gbc.p);
    if (grad_flux) pfv::adjoint_nl_grad_flux(cx, F, cx.nl_bc.p, z, cx.aj_phi.p, cx.aj_gq.p);
    if (grad_fluxfn)
      pfv::adjoint_nl_grad_fluxfn(cx, F, cx.pat_T, cx.valT_T.p, d_sink, d_q, cx.nl_bc.p, z, cx.aj_sB.p, cx.aj_gF.p);
  });
  h->stats.transport_nl_adjoint_ms = run.ms;
  h->stats.transport_nl_adjoint_steps = run.completed;
  h->stats.transport_nl_adjoint_core_iterations = run.core_total;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}

// ---- the adjoint of the saturation step with phase-carried components: one fused transposed sweep per step ------------
// In the frame of adjoint_steps with its own hooks, for it has two kinds of multipliers (lambda of the saturation in
// aj_lam / aj_lam2, mu of the components in aj_mu / aj_mu2) and two slabs (s in aj_sA / aj_sB, c in aj_cA / aj_cB): per
// step the slab (s^n, c^n), the slopes with the dry-row flag and the two right-hand sides fused with what the
// multipliers of step n + 1 add to the cell gradients; sweep_step_solve on mu and lambda jointly (sweep_row_nlc_t),
// the k + 1 pairs of norms and the flag in its ONE host read.  The last pass on slab 0 leaves grad_s0 and grad_c0.
pfv_status pfv_transport_adjoint_nl_multi(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                          int n_params, const double* bc_values, const double* accumulation,
                                          const double* sink, int k, const double* c_bc_values, const double* sorption,
                                          int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* s_loads,
                                          const double* c_loads, const double* s_states, const double* c_states,
                                          double rtol, int maxit, double* grad_s0, double* grad_c0, double* grad_source,
                                          double* grad_c_source, double* grad_accumulation, double* grad_sorption,
                                          double* grad_sink, double* grad_bc_values, double* grad_c_bc_values,
                                          double* grad_flux, double* grad_fluxfn, int32_t* steps_done,
                                          pfv_solve_info* last) {
  if (steps_done) *steps_done = 0;
  if (k < 1 || k > 64) return guarded(h, [&] { require(false, "k must lie in 1 .. 64"); });
  StepSetup S;
  const double* d_q = nullptr;
  size_t nc = 0, nf = 0;
  pfv::FluxFn F;
  pfv_status st = step_setup(h, S, steps_done, [&] {
    adjoint_nl_supported(h, fluxfn_kind, fluxfn_params, n_params, grad_fluxfn, bc_values, accumulation);
    require(c_bc_values, "c_bc_values is required");
    adjoint_check_counts(n_steps, rtol, maxit, s_loads || c_loads, "s_loads or c_loads is required");
    require((s_states && c_states) || n_steps == 0,
            "s_states (s^0 .. s^N) and c_states (c^0 .. c^N) are required: the step is linearised about them");
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    if ((int64_t)(k + 1) * (int64_t)std::max(nc, nf) >= (int64_t(1) << 31))
      throw Error(PFV_ERR_UNSUPPORTED, "(k + 1) x cells (faces) beyond int32 indices");
    // the observation: the saturation's loads first (they move to their own buffer), then the components'
    if (s_loads && n_steps > 0) {
      adjoint_take_loads(h, 1, n_steps, n_obs, obs_cells, s_loads);
      const size_t nl = (size_t)n_steps * (size_t)n_obs;
      if (nl) pfv::be_d2d(h->aj_sloads.ensure(nl), h->aj_loads.p, sizeof(double) * nl, h->stream);
    }
    adjoint_take_loads(h, k, c_loads ? n_steps : 0, n_obs, obs_cells, c_loads);
    if (q) vec_in(h, h->nl_q.ensure(nf), q, nf);
    vec_in(h, h->nl_bc.ensure(nf), bc_values, nf);
    vec_in(h, h->nl_acc.ensure(nc), accumulation, nc);
    if (sink) vec_in(h, h->nl_sink.ensure(nc), sink, nc);
    vec_in(h, h->nlc_cbc.ensure(k * nf), c_bc_values, k * nf);
    if (sorption) vec_in(h, h->nlc_ads_in.ensure(k * nc), sorption, k * nc);
    d_q = q ? h->nl_q.p : h->upw_q.p;
    pfv::upwind_face_cells(*h);
    // (the states are not checked: the accumulation stands in for s, zeros for c)
    pfv::be_memset(h->nlc_c_in.ensure(k * nc), 0, sizeof(double) * k * nc, h->stream);
    int32_t off[pfv::kNlChecks];
    pfv::sweep_nl_check_inputs(*h, d_q, h->nl_bc.p, h->nl_acc.p, sink ? h->nl_sink.p : nullptr, h->nl_acc.p, k,
                               sorption ? h->nlc_ads_in.p : nullptr, h->nlc_c_in.p, h->nlc_cbc.p, off);
    nl_inputs_refused(off, k, kNlStates);
    if (fluxfn_kind == PFV_FLUXFN_TABLE)
      be_h2d(h->nl_table.ensure((size_t)n_params), fluxfn_params, sizeof(double) * (size_t)n_params, h->stream);
    F = pfv::fluxfn_make(fluxfn_kind, fluxfn_params, n_params, h->nl_table.p);
    adjoint_system(h, S, d_q, h->nl_bc.p, n_obs, obs_cells);
    if (sorption) pfv::multi_interleave(*h, (int64_t)nc, k, h->nlc_ads_in.p, h->nlc_ads.ensure(k * nc));
    for (pfv::Buf<double>* b : {&h->aj_lam, &h->aj_lam2, &h->aj_prev, &h->aj_r, &h->aj_sA, &h->aj_sB, &h->aj_d, &h->aj_phi})
      b->ensure(nc);
    for (pfv::Buf<double>* b : {&h->aj_mu, &h->aj_mu2, &h->aj_muprev, &h->aj_rmu, &h->aj_cA, &h->aj_cB, &h->aj_state_in,
                                &h->mc_c})
      b->ensure(k * nc);
    pfv::be_memset(h->aj_mu.p, 0, sizeof(double) * k * nc, h->stream);  // mu^{N+1} = 0
    h->mc_nrm.ensure(2 * (size_t)(k + 1) + 1);  // the k + 1 pairs, then the word of the dry rows
  });
  if (st != PFV_OK) return st;

  const int K = k + 1;  // the norms' pairs: components 0 .. k - 1, then the saturation
  StepRun run;
  const double* d_sink = sink ? h->nl_sink.p : nullptr;
  const double* d_ads = sorption ? h->nlc_ads.p : nullptr;
  AdjointCall call{k, n_steps, n_obs, obs_cells, nullptr, nullptr, nullptr, nullptr, steps_done, last};
  call.saturation = k;
  call.grads = {{grad_s0, &h->aj_r, nc, GradLayout::plain, false},
                {grad_c0, &h->aj_rmu, k * nc, GradLayout::by_cell, false},
                {grad_source, &h->aj_gsrc, nc, GradLayout::plain},
                {grad_c_source, &h->aj_gcsrc, k * nc, GradLayout::by_cell},
                {grad_accumulation, &h->aj_gacc, nc, GradLayout::plain},
                {grad_sorption, &h->aj_gads, k * nc, GradLayout::by_cell},
                {grad_sink, &h->aj_gsink, nc, GradLayout::plain},
                {grad_bc_values, &h->aj_gbc, nf, GradLayout::plain},
                {grad_c_bc_values, &h->aj_gcbc, k * nf, GradLayout::plain},
                {grad_flux, &h->aj_gq, nf, GradLayout::plain},
                {grad_fluxfn, &h->aj_gF, 6, GradLayout::host}};
  call.stage = [&](int n) {  // s^n into aj_sB, c^n interleaved into aj_cB; aj_sA / aj_cA hold slab n + 1
    vec_in(h, h->aj_sB.p, s_states + (size_t)n * nc, nc);
    vec_in(h, h->aj_state_in.p, c_states + (size_t)n * k * nc, k * nc);
    pfv::multi_interleave(*h, (int64_t)nc, k, h->aj_state_in.p, h->aj_cB.p);
  };
  call.rhs = [&](int n, bool have_next) {
    pfv::pfv_ctx_impl& cx = *h;
    if (n == 0 && !have_next) {
      pfv::be_memset(cx.aj_r.p, 0, sizeof(double) * nc, cx.stream);
      pfv::be_memset(cx.aj_rmu.p, 0, sizeof(double) * k * nc, cx.stream);
      return;
    }
    if (n > 0) {
      int32_t* dry = reinterpret_cast<int32_t*>(cx.mc_nrm.p + 2 * K);
      pfv::be_memset(dry, 0x7f, sizeof(double), cx.stream);
      pfv::adjoint_nlc_slopes(cx, F, k, cx.aj_sB.p, cx.diag_t.p, d_sink, cx.nl_acc.p, d_ads, cx.aj_d.p, cx.aj_phi.p, dry);
    }
    pfv::adjoint_nlc_step_rhs(cx, k, cx.nl_acc.p, d_ads, cx.aj_sB.p, cx.aj_cB.p, cx.aj_sA.p, cx.aj_cA.p,
                              have_next ? cx.aj_lam.p : nullptr, cx.aj_mu.p, n > 0 && obs_cells ? cx.aj_slot.p : nullptr,
                              n > 0 && s_loads ? cx.aj_sloads.p + (size_t)(n - 1) * (size_t)n_obs : nullptr,
                              n > 0 && c_loads ? cx.aj_loads.p + (size_t)(n - 1) * k * (size_t)n_obs : nullptr,
                              n > 0 ? n_obs : 0, n == 0, grad_source ? cx.aj_gsrc.p : nullptr,
                              grad_c_source ? cx.aj_gcsrc.p : nullptr, grad_accumulation ? cx.aj_gacc.p : nullptr,
                              grad_sorption ? cx.aj_gads.p : nullptr, cx.aj_r.p, cx.aj_rmu.p);
  };
  call.swap = [&] {
    h->aj_lam.swap(h->aj_lam2);
    h->aj_mu.swap(h->aj_mu2);
    h->aj_sA.swap(h->aj_sB);
    h->aj_cA.swap(h->aj_cB);
  };
  st = adjoint_steps(h, S, call, run, [&](int n, double* z) -> pfv_status {
    pfv::pfv_ctx_impl& cx = *h;
    const pfv::Sweep& sw = *cx.sweep;
    const double* valT = cx.valT_T.p;
    const double *acc = cx.nl_acc.p, *d = cx.aj_d.p, *phi = cx.aj_phi.p, *diag = cx.diag_t.p, *s_n = cx.aj_sB.p;
    pfv::NlCompT C;  // the levels outside the core; Cc: the core level, with the previous iterate
    C.k = k;
    C.ads = d_ads;
    C.r = cx.aj_rmu.p;
    C.mu_next = cx.aj_mu.p;
    C.c = cx.aj_cB.p;
    C.mu = cx.aj_mu2.p;
    pfv::NlCompT Cc = C;
    Cc.mu_prev = cx.aj_muprev.p;
    Cc.lam_prev = cx.aj_prev.p;
    SweepSolve V{K, k, cx.mc_nrm.p, kAdjointSweep};
    V.levels = [&](int from, int to) {
      return pfv::sweep_apply_nlc_t(cx, sw, from, to, cx.pat_T, valT, diag, d_sink, acc, d, phi, s_n, cx.aj_r.p, z, C);
    };
    V.core_start = [&] {
      pfv::sweep_core_zero(cx, sw, 1, z);
      pfv::sweep_core_zero(cx, sw, k, C.mu);
    };
    V.core_step = [&] {
      pfv::sweep_core_copy(cx, sw, 1, z, cx.aj_prev.p);
      pfv::sweep_core_copy(cx, sw, k, C.mu, cx.aj_muprev.p);
      pfv::sweep_core_nlc_t(cx, sw, cx.pat_T, valT, diag, d_sink, acc, d, phi, s_n, cx.aj_r.p, z, Cc);
    };
    V.norms = [&](bool core_only) {
      pfv::sweep_norms_nlc_t(cx, sw, cx.pat_T, valT, d_sink, acc, d, phi, s_n, cx.aj_r.p, z, C, core_only, cx.mc_nrm.p);
    };
    V.flag_ends_core = true;  // (a dry row never settles)
    V.flagged = [&](int step, int32_t w) -> pfv_status {
      throw Error(PFV_ERR_ARGUMENT, "adjoint step " + std::to_string(step) + ": cell " + std::to_string(w / k) +
                                        ", component " + std::to_string(w % k) + " is dry (accumulation x s + sorption + "
                                        "f(s) x outflow is zero: the step does not determine the component there)");
    };
    return sweep_step_solve(h, V, run, rtol, maxit, n);
  }, [&](double* z) {
    pfv::pfv_ctx_impl& cx = *h;
    const double *mu = cx.aj_mu2.p, *s_n = cx.aj_sB.p, *c_n = cx.aj_cB.p, *phi = cx.aj_phi.p;
    if (grad_sink) pfv::adjoint_nlc_grad_sink(cx, k, z, mu, c_n, phi, cx.aj_gsink.p);
    if (grad_bc_values) pfv::adjoint_nlc_grad_bc(cx, F, k, d_q, cx.nl_bc.p, cx.nlc_cbc.p, z, mu, cx.aj_gbc.p);
    if (grad_c_bc_values) pfv::adjoint_nlc_grad_cbc(cx, F, k, d_q, cx.nl_bc.p, mu, cx.aj_gcbc.p);
    if (grad_flux) pfv::adjoint_nlc_grad_flux(cx, F, k, cx.nl_bc.p, cx.nlc_cbc.p, z, mu, phi, c_n, cx.aj_gq.p);
    if (grad_fluxfn)
      pfv::adjoint_nlc_grad_fluxfn(cx, F, cx.pat_T, cx.valT_T.p, d_sink, k, d_q, cx.nl_bc.p, cx.nlc_cbc.p, z, mu, s_n,
                                   c_n, cx.aj_gF.p);
  });
  h->stats.transport_nlc_adjoint_ms = run.ms;
  h->stats.transport_nlc_adjoint_steps = run.completed;
  h->stats.transport_nlc_adjoint_core_iterations = run.core_total;
  sweep_step_stats(h, n_steps > 0 ? run.launches : -1, S.order_ms);
  return st;
}


// ---- advection-diffusion on one handle (advdiff.inc) -----------------------------------------------------------
static void advdiff_supported(pfv_ctx* h) {
  require(h->have_grid, "pfv_set_grid first");
  if (h->periodic) throw pfv::Error(PFV_ERR_UNSUPPORTED, "advection-diffusion on periodic grids is not covered");
  if (h->shard) throw pfv::Error(PFV_ERR_UNSUPPORTED, "the advection-diffusion calls have no sharded form");
  if (h->subface_bc) throw pfv::Error(PFV_ERR_UNSUPPORTED, "conditions per sub-face are not covered");
}

static bool advdiff_is_active(const pfv_ctx* h) {
  return h->have_advdiff && h->have_system && h->have_adv_bD && active_is(h, PFV_MAT_ADVDIFF_SYSTEM);
}

pfv_status pfv_resident_flux(pfv_ctx* h, double** d_q, double* q_out) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_q_res, "no resident face flux on the handle (pfv_mpfa_face_flux)");
    if (q_out) vec_out(h, q_out, h->q_res.p, (size_t)h->nf);
    pfv::be_sync(h->stream);  // (a reader on another handle's stream must find it complete)
    if (d_q) *d_q = h->q_res.p;
  });
}

pfv_status pfv_advdiff_assemble(pfv_ctx* h, const double* q, double flux_scale, const double* bc_values,
                                const double* accumulation, const double* c_old, const double* source,
                                double* bound_rhs_out) {
  return guarded(h, [&] {
    advdiff_supported(h);
    require(h->have_numeric && h->have_params && h->filled[PFV_MAT_FLUX] && h->filled[PFV_MAT_BOUND_FLUX],
            "discretize the diffusion first (pfv_mpfa_discretize / pfv_tpfa_discretize)");
    require(flux_scale > 0.0 && flux_scale < HUGE_VAL, "flux_scale must be positive and finite");
    require(q || h->have_q_res, "no face flux given and no resident face flux on the handle (pfv_mpfa_face_flux)");
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc;
    if (active_is(h, PFV_MAT_ADVDIFF_SYSTEM)) h->active.valid = false;
    h->have_advdiff = false;
    h->filled[PFV_MAT_ADVDIFF_SYSTEM] = false;
    h->advdiff_zero_diag = -1;
    double* d_q = h->adv_q.ensure(nf);
    if (q) vec_in(h, d_q, q, nf);
    else pfv::be_d2d(d_q, h->q_res.p, nf * sizeof(double), s);
    h->have_adv_acc = accumulation != nullptr;
    h->have_adv_src = source != nullptr;
    if (accumulation) vec_in(h, h->adv_acc.ensure(nc), accumulation, nc);
    if (source) vec_in(h, h->adv_src.ensure(nc), source, nc);
    const double* d_cold = nullptr;
    if (c_old) {
      vec_in(h, h->adv_c.ensure(nc), c_old, nc);
      d_cold = h->adv_c.p;
    }
    pfv::Timer tm;
    if (!h->have_system) {  // div @ flux_D: once per discretization, by the flow assembly
      pfv::assemble_system(*h);
      h->have_adv_bD = false;
      values_changed(h, Windows::consume);  // (PFV_MAT_SYSTEM's)
      h->have_system = true;      // PFV_MAT_SYSTEM and its diagonal hold div @ flux ...
      h->have_flow_rhs = false;   // ... but no flow right-hand side was formed with them
    }
    require(bc_values || h->have_adv_bD, "bc_values is required in the first call after a discretization");
    if (bc_values) vec_in(h, h->adv_bc.ensure(nf), bc_values, nf);
    tm.start(s);
    if (!h->have_adv_bD) pfv::advdiff_check_pattern(*h);
    if (bc_values || !h->have_adv_bD) pfv::advdiff_diffusion_rhs(*h, h->adv_bc.p);
    h->have_adv_bD = true;
    h->adv_w = flux_scale;
    pfv::advdiff_refresh(*h, d_q, flux_scale, h->adv_bc.p, h->have_adv_acc ? h->adv_acc.p : nullptr, d_cold,
                         h->have_adv_src ? h->adv_src.p : nullptr);
    h->stats.advdiff_assemble_ms = tm.stop(s);
    sweep_note_assembly(h, PFV_MAT_ADVDIFF_SYSTEM, d_q);
    if (bound_rhs_out) vec_out(h, bound_rhs_out, h->adv_bref.p, nc);
    pfv::be_sync(s);
    h->have_advdiff = true;
    values_changed(h, Windows::keep);  // (S shares pat_A with div @ flux; the aggregate maps stay too)
    activate(h, h->pat_A, h->val[PFV_MAT_ADVDIFF_SYSTEM].p, h->adv_diag.p, h->adv_rhs.p, h->nc, 1, true);
  });
}

pfv_status pfv_advdiff_advance(pfv_ctx* h, int n_steps, int method, double rtol, int maxit, double* c,
                               int32_t* steps_done, pfv_solve_info* last) {
  static const StepLoop loop{&pfv_ctx::adv_c, &pfv_ctx::adv_keep, pfv::advdiff_step_rhs, false, true};
  StepTotals tot;
  const pfv_status st = advance_steps(h, loop, [&] {
    advdiff_supported(h);
    require(advdiff_is_active(h), "pfv_advdiff_assemble first (the advection-diffusion system must be the active one)");
    require(n_steps >= 0 && c != nullptr, "bad argument");
    require(method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES (the matrix is not symmetric)");
    require(h->precond == PFV_PRECOND_JACOBI || h->precond == PFV_PRECOND_AMG || h->precond == PFV_PRECOND_SWEEP,
            "the advection-diffusion step takes PFV_PRECOND_JACOBI, PFV_PRECOND_AMG or PFV_PRECOND_SWEEP");
  }, n_steps, method, rtol, maxit, c, steps_done, last, tot);
  if (tot.ran) {
    h->stats.advdiff_advance_ms = tot.ms;
    h->stats.advdiff_iterations = tot.iterations;
    h->stats.advdiff_gmres_retries = tot.gmres_retries;
    h->stats.advdiff_precond_fallbacks = tot.precond_fallbacks;
    if (h->precond == PFV_PRECOND_SWEEP) h->stats.sweep_order_ms = tot.order_ms;
  }
  return st;
}

pfv_status pfv_advdiff_face_flux(pfv_ctx* h, const double* c, double* out) {
  return guarded(h, [&] {
    advdiff_supported(h);
    require(h->have_advdiff && h->have_system && h->have_adv_bD && h->have_numeric,
            "pfv_advdiff_assemble first (and no new discretization since)");
    require(c && out, "null argument");
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc;
    pfv::Buf<double> in_;
    double* d_c = in_.ensure(nc + nf);
    double* d_out = d_c + nc;
    vec_in(h, d_c, c, nc);
    pfv::advdiff_face_flux(*h, d_c, d_out);
    vec_out(h, out, d_out, nf);
    pfv::be_sync(s);  // (the staging buffer is freed on return)
  });
}

// The cell -> sub-cell map of the exact gradients (mpfa_adjoint.inc), kept under the topology digest.  true: built now.
static bool adj_ensure_cell_map(pfv_ctx* h) {
  const unsigned long long key = h->topo_key ? h->topo_key : pfv::topology_digest(*h);
  if (h->adj_map_key != 0 && h->adj_map_key == key) return false;
  h->adj_map_key = 0;
  pfv::adj_cell_map(*h);
  h->adj_map_key = key;
  ++h->stats.flow_adjoint_exact_map_builds;
  return true;
}

// ---- the adjoint of the advection-diffusion step (advdiff_adjoint.inc) ---------------------------------------------
// The checks and the set-up run as the `checks` of advance_steps and end with (pat_A, S^T, diag, ada_rhs) as the active
// system; the loop is advance_steps itself -- the state is lambda, step `step` is n = N - step --, with the right-hand
// side and the two accumulation passes as its hooks; the products that need the sums over the steps follow the loop.
// (grad_exact: the additional output of pfv_advdiff_adjoint_exact, nullptr for pfv_advdiff_adjoint -- whose path through
// this body is the one it always took.  With an MPFA diffusion the after hook also writes z^n = -cell_faces lambda^n into
// slab m of a ring of B = exact_batch slabs and notes c^n; every B accepted steps, and after the last one, ONE pass over
// the interaction regions (pfv::advdiff_adjoint_exact_batch) adds the pending states to the running sums per sub-cell.)
enum { kAdvdiffExactBatch = 32 };  // the default B
static pfv_status advdiff_adjoint_call(pfv_ctx* h, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                       const double* loads, const double* states, int method, double rtol, int maxit,
                                       double* grad_c0, double* grad_source, double* grad_bc_values,
                                       double* grad_accumulation, double* grad_flux, double* grad_flux_scale,
                                       double* grad_conductivity, double* multipliers_out, int32_t* steps_done,
                                       pfv_solve_info* last, double* grad_exact, int exact_batch) {
  static const StepLoop loop{&pfv_ctx::ada_lam, &pfv_ctx::ada_keep, nullptr, false, true};
  const int none = 0x7f7f7f7f;
  const int N = n_steps;
  const bool want_sq = grad_flux || grad_flux_scale;
  const bool want_Lam = grad_source || grad_bc_values;
  const bool cell_pass = want_Lam || grad_accumulation || multipliers_out;
  // (a TPFA diffusion: the two-point gradient is the exact one, formed whether or not grad_conductivity was asked for)
  bool want_zw = grad_conductivity != nullptr, face_pass = want_sq || want_zw;
  bool region = false;  // the interaction-region passes run
  int B = 0, pend = 0, n_first = 0, passes = 0;
  std::vector<std::unique_ptr<pfv::Timer>> exact_tm;
  double exact_ms = 0.0;
  bool activated = false, on_dev = false;
  size_t nc = 0, nf = 0;
  int32_t *first = nullptr, *last_hf = nullptr, *ecell = nullptr;
  const int32_t* slot = nullptr;
  const double *acc = nullptr, *cn = nullptr, *cprev = nullptr;
  std::unique_ptr<pfv::Timer> whole;
  std::vector<std::unique_ptr<pfv::Timer>> pass_tm;
  double pass_ms = 0.0;
  int32_t done = 0;
  StepTotals tot;
  StepHooks hooks;
  hooks.rhs = [&](int step) {
    const int n = N - step;
    pfv::pfv_ctx_impl& cx = *h;
    if (states && (face_pass || grad_accumulation || region)) {  // c^n and c^{n-1}: in place on the device, else one slab per step
      if (on_dev) {
        cn = states + (size_t)n * nc;
        cprev = states + (size_t)(n - 1) * nc;
      } else if (grad_accumulation) {  // ada_sA holds c^n (staged by the step before, or ahead of the loop)
        be_h2d(cx.ada_sB.p, states + (size_t)(n - 1) * nc, sizeof(double) * nc, cx.stream);
        cn = cx.ada_sA.p;
        cprev = cx.ada_sB.p;
      } else {  // (with the region passes: staged where the batch reads it)
        double* slab = region ? cx.ada_sr.p + (size_t)pend * nc : cx.ada_sA.p;
        be_h2d(slab, states + (size_t)n * nc, sizeof(double) * nc, cx.stream);
        cn = slab;
      }
    }
    pfv::advdiff_adjoint_rhs(cx, slot, cx.aj_loads.p + (size_t)(n - 1) * (size_t)n_obs, acc, cx.ada_lam.p, cx.ada_rhs.p);
  };
  hooks.after = [&](int step) {
    const int n = N - step;
    pfv::pfv_ctx_impl& cx = *h;
    pass_tm.emplace_back(std::make_unique<pfv::Timer>());
    pfv::Timer& tm = *pass_tm.back();
    tm.start(cx.stream);
    if (face_pass)
      pfv::advdiff_adjoint_faces(cx, first, last_hf, ecell, cx.adv_q.p, cx.adv_bc.p, cx.ada_lam.p, cn,
                                 want_sq ? cx.ada_sq.p : nullptr, want_zw ? cx.ada_zw.p : nullptr);
    if (cell_pass)
      pfv::advdiff_adjoint_cells(cx, cx.ada_lam.p, cprev, cn, want_Lam ? cx.ada_Lam.p : nullptr,
                                 grad_accumulation ? cx.ada_gacc.p : nullptr,
                                 multipliers_out ? cx.ada_mult.p + (size_t)(n - 1) * nc : nullptr);
    if (region) pfv::advdiff_adjoint_exact_load(cx, first, last_hf, ecell, cx.ada_lam.p, cx.ada_zr.p + (size_t)pend * nf);
#ifdef PFV_EMULATE
    pass_ms += tm.stop(cx.stream);
#else
    tm.mark(cx.stream);  // (read after the loop: the step adds no host read)
#endif
    if (region) {  // state m = pend of the batch is step n = n_first - m
      if (!on_dev && grad_accumulation) pfv::be_d2d(cx.ada_sr.p + (size_t)pend * nc, cn, sizeof(double) * nc, cx.stream);
      if (pend == 0) n_first = n;
      if (++pend == B || n == 1) {
        exact_tm.emplace_back(std::make_unique<pfv::Timer>());
        pfv::Timer& te = *exact_tm.back();
        te.start(cx.stream);
        passes += pfv::advdiff_adjoint_exact_batch(cx, cx.ada_st.p, on_dev ? states + (size_t)n_first * nc : cx.ada_sr.p,
                                                   on_dev ? -(int64_t)nc : (int64_t)nc, cx.ada_zr.p, cx.adv_bc.p, pend);
#ifdef PFV_EMULATE
        exact_ms += te.stop(cx.stream);
#else
        te.mark(cx.stream);
#endif
        pend = 0;
      }
    }
    if (states && !on_dev && grad_accumulation) cx.ada_sA.swap(cx.ada_sB);
    ++done;
  };
  pfv_status st = advance_steps(h, loop, [&] {
    advdiff_supported(h);
    require(advdiff_is_active(h), "pfv_advdiff_assemble first (the advection-diffusion system must be the active one)");
    require(n_steps >= 0, "n_steps must not be negative");
    require(method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES (the matrix is not symmetric)");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    if (h->precond == PFV_PRECOND_SWEEP)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_SWEEP is not covered by the advection-diffusion adjoint: the "
                                            "substitution in reverse flow order on S^T is a later pull request; select "
                                            "PFV_PRECOND_AMG or PFV_PRECOND_JACOBI");
    require(h->precond == PFV_PRECOND_JACOBI || h->precond == PFV_PRECOND_AMG,
            "the advection-diffusion adjoint takes PFV_PRECOND_JACOBI or PFV_PRECOND_AMG");
    require(states || !grad_accumulation, "grad_accumulation needs states (c^0 .. c^N)");
    require(states || !grad_flux, "grad_flux needs states (c^0 .. c^N)");
    require(states || !grad_flux_scale, "grad_flux_scale needs states (c^0 .. c^N)");
    require(states || !grad_conductivity, "grad_conductivity needs states (c^0 .. c^N)");
    require(states || !grad_exact, "grad_conductivity_exact needs states (c^0 .. c^N)");
    require(exact_batch >= 0, "exact_batch must not be negative");
    require(loads || n_steps == 0 || n_obs == 0, "loads is required");
    if (!h->tpfa_mode && !h->rows_complete)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "the advection-diffusion adjoint does not cover a partial discretization "
                                            "(the rows of the other faces are zero)");
    if (h->pat_A.nnz >= (int64_t(1) << 31) || h->pat_bound.nnz >= (int64_t(1) << 31))
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "the advection-diffusion adjoint needs patterns of div flux and bound_flux "
                                            "below 2^31 entries");
    auto s = h->stream;
    nc = (size_t)h->nc;
    nf = (size_t)h->nf;
    const size_t ncf = (size_t)h->ncf;
    on_dev = h->vectors_on_device;
    int32_t robin = none, internal = none;
    pfv::advdiff_adjoint_check_faces(*h, robin, internal);
    if (robin != none)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "face " + std::to_string(robin) + " carries a Robin condition: the "
                                            "advection-diffusion adjoint covers Dirichlet and Neumann faces");
    if (internal != none)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "face " + std::to_string(internal) + " is flagged PFV_BC_INTERNAL: the "
                                            "advection-diffusion adjoint does not cover internal boundaries");
    adjoint_take_loads(h, 1, n_steps, n_obs, obs_cells, loads);
    adjoint_take_slots(h, n_obs, obs_cells);
    slot = obs_cells ? h->aj_slot.p : nullptr;
    acc = h->have_adv_acc ? h->adv_acc.p : nullptr;
    if (grad_exact && h->tpfa_mode) want_zw = face_pass = true;
    region = grad_exact && !h->tpfa_mode;
    if (region) {  // (a region too large for the LDS: refused before anything runs)
      pfv::adj_check_lds(*h);
      pfv::Timer tm;
      tm.start(s);
      if (adj_ensure_cell_map(h)) h->stats.flow_adjoint_exact_map_ms = tm.stop(s);
      B = std::max(1, std::min(exact_batch ? exact_batch : (int)kAdvdiffExactBatch, N));
    }
    whole = std::make_unique<pfv::Timer>();
    whole->start(s);
    // ---- what belongs to the patterns and the grid: the half-face lists, the column maps, the transposed positions
    int32_t* half = h->fa_half.ensure(2 * nf + ncf);
    first = half;
    last_hf = half + nf;
    ecell = half + 2 * nf;
    pfv::flow_adjoint_half_faces(*h, first, last_hf, ecell);
    pfv::upwind_face_cells(*h);
    const size_t nnzA = (size_t)std::max<int64_t>(h->pat_A.nnz, 1);
    if (grad_bc_values && !h->have_cmap) {
      pfv::colmap_build(*h, h->pat_flux, h->cmap_flux);
      pfv::colmap_build(*h, h->pat_bound, h->cmap_bound);
      h->have_cmap = true;
      ++h->stats.flow_adjoint_map_builds;
    }
    if (!h->have_tpos_A) {
      pfv::sweep_transpose_positions(*h, h->pat_A, h->tpos_A.ensure(nnzA), "div flux");
      h->have_tpos_A = true;
    }
    // ---- the accumulators and the slabs
    auto zeros = [&](pfv::Buf<double>& b, size_t n) { pfv::be_memset(b.ensure(std::max<size_t>(n, 1)), 0, sizeof(double) * n, s); };
    h->ada_rhs.ensure(nc);
    if (want_Lam) zeros(h->ada_Lam, nc);
    if (grad_accumulation) zeros(h->ada_gacc, nc);
    if (want_sq) zeros(h->ada_sq, nf);
    if (want_zw) zeros(h->ada_zw, nf);
    if (multipliers_out) zeros(h->ada_mult, (size_t)N * nc);
    if (region) {  // the ring of loads, the ring of staged states, the running sums per sub-cell, the status words
      const size_t nsub = (size_t)std::max<int64_t>(h->nh / h->nd * h->nd * h->nd, 1);
      h->ada_zr.ensure((size_t)B * std::max<size_t>(nf, 1));
      if (!on_dev) h->ada_sr.ensure((size_t)B * std::max<size_t>(nc, 1));
      pfv::be_memset(h->adj_sub.ensure(nsub), 0, sizeof(double) * nsub, s);
      pfv::be_memset(h->ada_st.ensure(16), 0, sizeof(int32_t) * 4, s);
    }
    if (states && !on_dev && (face_pass || grad_accumulation || region)) {
      h->ada_sA.ensure(nc);
      h->ada_sB.ensure(nc);
      if (grad_accumulation && N > 0) be_h2d(h->ada_sA.p, states + (size_t)N * nc, sizeof(double) * nc, s);  // c^N
    }
    // ---- S^T on the pattern of S: the active system of all steps (with AMG: one hierarchy, set up by the first)
    double* valT = h->fa_valT.ensure(nnzA);
    pfv::sweep_transpose_values(*h, h->pat_A.nnz, h->tpos_A.p, h->val[PFV_MAT_ADVDIFF_SYSTEM].p, valT);
    h->active.valid = false;
    h->have_advdiff = false;  // (the call ends without an active system: pfv_advdiff_assemble is asked for)
    activated = true;
    values_changed(h, Windows::keep);
    activate(h, h->pat_A, valT, h->adv_diag.p, h->ada_rhs.p, h->nc, 1, true);
  }, n_steps, method, rtol, maxit, nullptr, nullptr, last, tot, &hooks);
  if (steps_done) *steps_done = done;
  if (!tot.ran) return st;
  const std::string err = h->err;
  const pfv_status st2 = guarded(h, [&] {
    pfv::pfv_ctx_impl& cx = *h;
    auto s = cx.stream;
    if (activated) cx.active.valid = false;
#ifndef PFV_EMULATE
    for (auto& t : pass_tm) pass_ms += t->elapsed_after_sync();
#endif
    pass_tm.clear();
#ifndef PFV_EMULATE
    for (auto& t : exact_tm) exact_ms += t->elapsed_after_sync();
#endif
    exact_tm.clear();
    if (st == PFV_OK) {
      const size_t ncf = (size_t)cx.ncf;
      pfv::Buf<double> inv_, gk_, ge_;
      double* ge = nullptr;
      if (region) {  // the status words of all passes, read once; then the cell sum
        int32_t sth[4];
        be_d2h(sth, cx.ada_st.p, sizeof(sth), s);
        pfv::adj_throw_status(sth);
        pfv::Timer tm;
        tm.start(s);
        ge = ge_.ensure(9 * nc);
        pfv::adj_cell_sum(cx, cx.adj_sub.p, ge);
        exact_ms += tm.stop(s);
      }
      double* work = cx.ada_work.ensure(2 * nf + pfv::kAdaParts + 1);
      double *Y = work, *gb = work + nf, *parts = work + 2 * nf, *total = parts + pfv::kAdaParts;
      if (grad_bc_values) {
        pfv::advdiff_adjoint_face_sum(cx, first, last_hf, ecell, cx.ada_Lam.p, Y);
        pfv::spmv_transposed(cx, cx.cmap_bound, cx.val[PFV_MAT_BOUND_FLUX].p, Y, gb);
        pfv::advdiff_adjoint_grad_bc(cx, cx.adv_q.p, cx.adv_w, Y, gb);
      }
      double* gk = nullptr;
      if (want_zw) {
        gk = gk_.ensure(9 * nc);
        pfv::flow_adjoint_grad_perm(cx, first, last_hf, cx.ada_zw.p, inv_.ensure(std::max<size_t>(ncf, 1)), gk);
      }
      if (want_sq) pfv::advdiff_adjoint_flux_out(cx, cx.adv_q.p, cx.adv_w, cx.ada_sq.p, parts, total);
      if (grad_c0) pfv::advdiff_adjoint_grad_c0(cx, acc, cx.ada_lam.p, cx.ada_rhs.p);
      h->stats.advdiff_adjoint_ms = whole->stop(s);
      if (grad_c0) vec_out(h, grad_c0, cx.ada_rhs.p, nc);
      if (grad_source) vec_out(h, grad_source, cx.ada_Lam.p, nc);
      if (grad_bc_values) vec_out(h, grad_bc_values, gb, nf);
      if (grad_accumulation) vec_out(h, grad_accumulation, cx.ada_gacc.p, nc);
      if (grad_flux) vec_out(h, grad_flux, cx.ada_sq.p, nf);
      if (grad_flux_scale) be_d2h(grad_flux_scale, total, sizeof(double), s);  // (host memory, as the scale itself is)
      if (grad_conductivity) vec_out(h, grad_conductivity, gk, 9 * nc);
      if (grad_exact) vec_out(h, grad_exact, ge ? ge : gk, 9 * nc);
      if (multipliers_out) vec_out(h, multipliers_out, cx.ada_mult.p, (size_t)N * nc);
    } else {
      h->stats.advdiff_adjoint_ms = whole->stop(s);
    }
    pfv::be_sync(s);  // (the staging buffers are freed on return)
    whole.reset();
  });
  h->stats.advdiff_adjoint_steps = done;
  h->stats.advdiff_adjoint_iterations = tot.iterations;
  h->stats.advdiff_adjoint_gmres_retries = tot.gmres_retries;
  h->stats.advdiff_adjoint_precond_fallbacks = tot.precond_fallbacks;
  h->stats.advdiff_adjoint_accumulate_ms = pass_ms;
  h->stats.advdiff_adjoint_exact_ms = exact_ms;
  h->stats.advdiff_adjoint_exact_passes = passes;
  h->stats.advdiff_adjoint_exact_batch = B;
  return step_status(h, st, err, st2);
}

pfv_status pfv_advdiff_adjoint(pfv_ctx* h, int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* loads,
                               const double* states, int method, double rtol, int maxit, double* grad_c0,
                               double* grad_source, double* grad_bc_values, double* grad_accumulation,
                               double* grad_flux, double* grad_flux_scale, double* grad_conductivity,
                               double* multipliers_out, int32_t* steps_done, pfv_solve_info* last) {
  return advdiff_adjoint_call(h, n_steps, n_obs, obs_cells, loads, states, method, rtol, maxit, grad_c0, grad_source,
                              grad_bc_values, grad_accumulation, grad_flux, grad_flux_scale, grad_conductivity,
                              multipliers_out, steps_done, last, nullptr, 0);
}

pfv_status pfv_advdiff_adjoint_exact(pfv_ctx* h, int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* loads,
                                     const double* states, int method, double rtol, int maxit, double* grad_c0,
                                     double* grad_source, double* grad_bc_values, double* grad_accumulation,
                                     double* grad_flux, double* grad_flux_scale, double* grad_conductivity,
                                     double* multipliers_out, int32_t* steps_done, pfv_solve_info* last,
                                     double* grad_conductivity_exact, int exact_batch) {
  return advdiff_adjoint_call(h, n_steps, n_obs, obs_cells, loads, states, method, rtol, maxit, grad_c0, grad_source,
                              grad_bc_values, grad_accumulation, grad_flux, grad_flux_scale, grad_conductivity,
                              multipliers_out, steps_done, last, grad_conductivity_exact, exact_batch);
}

pfv_status pfv_mpsa_set_params(pfv_ctx* h, const double* stiffness_99n, const double* cell_volumes,
                               const uint8_t* bc_dir_bits, const uint8_t* bc_neu_bits, double eta) {
  return guarded(h, [&] {
    require(h->have_grid, "pfv_set_grid must be called first");
    require(stiffness_99n && cell_volumes && bc_dir_bits && bc_neu_bits, "null parameter array");
    auto s = h->stream;
    upload(h->stiff, stiffness_99n, 81 * (size_t)h->nc, s);
    upload(h->cvol, cell_volumes, (size_t)h->nc, s);
    upload(h->bc_dirbits, bc_dir_bits, (size_t)h->nf, s);
    upload(h->bc_neubits, bc_neu_bits, (size_t)h->nf, s);
    h->have_mpsa_robin = false;
    h->have_mpsa_eta_sub = false;
    h->mpsa_hf_on = false;
    h->have_mpsa_hf_eta_sub = false;
    h->have_mpsa_basis = false;
    h->have_mpsa_basis_sub = false;
    h->mpsa_subface_bc = false;
    h->mpsa_eta = eta;
    h->have_mpsa_params = true;
    h->have_mpsa_numeric = h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_robin(pfv_ctx* h, const uint8_t* bc_rob_bits, const double* robin_weight_ddn) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    auto s = h->stream;
    h->have_mpsa_robin = false;
    if (!bc_rob_bits) return;
    const size_t nf = (size_t)h->nf, n2 = (size_t)h->nd * h->nd;
    upload(h->bc_robbits, bc_rob_bits, nf, s);
    if (robin_weight_ddn) {
      upload(h->mpsa_robw, robin_weight_ddn, n2 * nf, s);
    } else {
      std::vector<double> eye(n2 * nf, 0.0);
      for (int i = 0; i < h->nd; ++i)
        for (size_t f = 0; f < nf; ++f) eye[((size_t)h->nd * i + i) * nf + f] = 1.0;
      upload(h->mpsa_robw, eye.data(), n2 * nf, s);
    }
    h->have_mpsa_robin = true;
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_subface_eta(pfv_ctx* h, const double* eta_subface) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    h->have_mpsa_eta_sub = false;
    if (eta_subface) {
      upload(h->mpsa_eta_sub, eta_subface, (size_t)h->nsf, h->stream);
      h->have_mpsa_eta_sub = true;
    }
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_reconstruction_eta(pfv_ctx* h, int on, double hf_eta) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    require(!on || (hf_eta >= 0.0 && hf_eta < 1.0), "reconstruction_eta must lie in [0, 1)");
    h->mpsa_hf_on = on != 0;
    h->mpsa_hf_eta = hf_eta;
    h->have_mpsa_hf_eta_sub = false;
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_reconstruction_eta_subface(pfv_ctx* h, const double* hf_eta_subface) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    h->have_mpsa_hf_eta_sub = false;
    h->mpsa_hf_on = hf_eta_subface != nullptr;
    if (hf_eta_subface) {
      if (!h->have_topology) {  // the sub-face count is known from the topology
        pfv::build_topology(*h);
        pfv::build_symbolic(*h);
        h->tpfa_mode = false;
        h->have_mpsa_symbolic = false;
        h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
        h->have_numeric = h->have_system = false;
      }
      upload(h->mpsa_hf_eta_sub, hf_eta_subface, (size_t)h->nsf, h->stream);
      h->have_mpsa_hf_eta_sub = true;
    }
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_basis(pfv_ctx* h, const double* basis_ddn) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    h->have_mpsa_basis = false;
    if (basis_ddn) {
      upload(h->mpsa_basis, basis_ddn, (size_t)h->nd * h->nd * (size_t)h->nf, h->stream);
      h->have_mpsa_basis = true;
    }
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_set_subface_bc(pfv_ctx* h, const uint8_t* bc_dir_bits_sub, const uint8_t* bc_neu_bits_sub,
                                   const uint8_t* bc_rob_bits_sub, const double* robin_weight_dds) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "pfv_mpsa_set_params first");
    h->mpsa_subface_bc = false;
    h->have_mpsa_basis_sub = false;
    h->have_mpsa_numeric = h->have_mech_system = false;
    if (!bc_dir_bits_sub) return;  // back to conditions per face
    require(bc_neu_bits_sub != nullptr, "null parameter array");
    require(!h->have_mpsa_basis, "conditions per sub-face take their basis per sub-face: pfv_mpsa_set_subface_basis");
    require(h->biot_nalpha == 0, "conditions per sub-face with Biot coupling terms are not covered");
    auto s = h->stream;
    if (!h->have_topology) {  // the sub-face count is known from the topology
      pfv::build_topology(*h);
      pfv::build_symbolic(*h);
      h->tpfa_mode = false;
      h->have_mpsa_symbolic = false;
      h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
      h->have_numeric = h->have_system = false;
    }
    const size_t nsf = (size_t)h->nsf, n2 = (size_t)h->nd * h->nd;
    upload(h->bc_dirbits_sub, bc_dir_bits_sub, nsf, s);
    upload(h->bc_neubits_sub, bc_neu_bits_sub, nsf, s);
    h->have_mpsa_robin_sub = bc_rob_bits_sub != nullptr;
    if (bc_rob_bits_sub) {
      upload(h->bc_robbits_sub, bc_rob_bits_sub, nsf, s);
      if (robin_weight_dds) {
        upload(h->mpsa_robw_sub, robin_weight_dds, n2 * nsf, s);
      } else {
        std::vector<double> eye(n2 * nsf, 0.0);
        for (int i = 0; i < h->nd; ++i)
          for (size_t f = 0; f < nsf; ++f) eye[((size_t)h->nd * i + i) * nsf + f] = 1.0;
        upload(h->mpsa_robw_sub, eye.data(), n2 * nsf, s);
      }
    }
    h->mpsa_subface_bc = true;
  });
}

pfv_status pfv_mpsa_set_subface_basis(pfv_ctx* h, const double* basis_dds) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params && h->mpsa_subface_bc, "pfv_mpsa_set_subface_bc first");
    h->have_mpsa_basis_sub = false;
    if (basis_dds) {
      upload(h->mpsa_basis_sub, basis_dds, (size_t)h->nd * h->nd * (size_t)h->nsf, h->stream);
      h->have_mpsa_basis_sub = true;
    }
    h->have_mpsa_numeric = false;
    h->have_mech_system = false;
  });
}

pfv_status pfv_mpsa_discretize(pfv_ctx* h, uint32_t flags) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "grid and MPSA parameters must be set before discretize");
    auto s = h->stream;
    pfv::Timer tm;
    if (!h->have_topology || !h->have_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) {
      tm.start(s);
      pfv::build_topology(*h);
      h->stats.topology_ms = tm.stop(s);
      tm.start(s);
      // (a rebuilt topology that is proved equal to the one the patterns were built from keeps them -- and with them
      // their block expansions of mpsa_symbolic, functions of those patterns alone; see symbolic_outputs_still_valid)
      const bool had_mpsa_symbolic = h->have_mpsa_symbolic;
      if (symbolic_outputs_still_valid(h)) {
        h->stats.symbolic_ms = tm.stop(s);
        h->have_mpsa_symbolic = had_mpsa_symbolic;
        h->have_numeric = h->have_system = false;
      } else {
      pfv::build_symbolic(*h);
      h->stats.symbolic_ms = tm.stop(s);
      h->tpfa_mode = false;
      h->have_mpsa_symbolic = false;
      h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
      h->have_numeric = h->have_system = false;
      }
    }
    if (!h->have_mpsa_symbolic) {
      tm.start(s);
      pfv::mpsa_symbolic(*h);
      h->stats.symbolic_ms += tm.stop(s);
      h->have_biot_symbolic = false;
    }
    if (h->biot_nalpha > 0 && !h->have_biot_symbolic) pfv::biot_symbolic(*h);
    if (h->mpsa_subface_bc && !h->have_mpsa_sub_symbolic) {
      require(h->biot_nalpha == 0, "conditions per sub-face with Biot coupling terms are not covered");
      tm.start(s);
      pfv::mpsa_subface_symbolic(*h);
      h->stats.symbolic_ms += tm.stop(s);
    }
    tm.start(s);
    pfv::mpsa_run_node_kernel(*h);
    h->stats.node_ms = tm.stop(s);
    tm.start(s);
    pfv::mpsa_run_face_kernel(*h);
    if (h->mpsa_subface_bc) pfv::mpsa_run_subface_kernel(*h);
    h->stats.face_ms = tm.stop(s);
    h->have_mpsa_numeric = true;
    h->rows_complete_m = true;
    h->have_mech_system = false;
    h->filled[PFV_MAT_MECH_SYSTEM] = false;
  });
}

pfv_status pfv_mpsa_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces, const int32_t* faces,
                                     int keep_other_rows) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "grid and MPSA parameters must be set before discretize");
    require(n_faces >= 0 && (n_faces == 0 || faces), "bad face list");
    require(!keep_other_rows || h->rows_complete_m,
            "update of a discretization that was never computed on this handle");
    require(!h->mpsa_subface_bc, "partial discretization with conditions per sub-face is not covered");
    for (int64_t i = 0; i < n_faces; ++i)
      require(faces[i] >= 0 && faces[i] < h->nf, "face index out of range");
    auto s = h->stream;
    pfv::Timer tm;
    if (!h->have_topology || !h->have_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) {
      require(!keep_other_rows, "the topology cannot be rebuilt under an update");
      pfv::build_topology(*h);
      pfv::build_symbolic(*h);
      h->tpfa_mode = false;
      h->have_mpsa_symbolic = false;
      h->have_sub_symbolic = h->have_mpsa_sub_symbolic = false;
      h->have_numeric = h->have_system = false;
    }
    if (!h->have_mpsa_symbolic) {
      pfv::mpsa_symbolic(*h);
      h->have_biot_symbolic = false;
    }
    if (h->biot_nalpha > 0 && !h->have_biot_symbolic) pfv::biot_symbolic(*h);
    int32_t* sub = h->face_subset.ensure(std::max<int64_t>(n_faces, 1));
    uint8_t* act = h->node_active.ensure(h->nn);
    pfv::be_h2d(sub, faces, sizeof(int32_t) * (size_t)n_faces, s);
    pfv::be_memset(act, 0, (size_t)h->nn, s);
    const int32_t* fn_ptr = h->fn_ptr;
    const int32_t* fn_idx = h->fn_idx;
    pfv::parallel_for(s, n_faces, PFV_LAMBDA(int64_t i) {
      const int f = sub[i];
      for (int e = fn_ptr[f]; e < fn_ptr[f + 1]; ++e) act[fn_idx[e]] = 1;
    });
    tm.start(s);
    pfv::mpsa_run_node_kernel(*h, act);
    h->stats.node_ms = tm.stop(s);
    if (!keep_other_rows) {
      h->rows_complete_m = false;
      for (int m = PFV_MAT_STRESS; m <= PFV_MAT_BOUND_DISPLACEMENT_FACE; ++m) {
        const int64_t nnz = h->pattern_of(m).nnz;
        double* v = h->val[m].ensure(std::max<int64_t>(nnz, 1));
        pfv::be_memset(v, 0, sizeof(double) * (size_t)nnz, s);
      }
    }
    tm.start(s);
    pfv::mpsa_run_face_kernel(*h, sub, n_faces);
    h->stats.face_ms = tm.stop(s);
    h->have_mpsa_numeric = true;
    h->have_mech_system = false;
    h->filled[PFV_MAT_MECH_SYSTEM] = false;
  });
}

pfv_status pfv_biot_set_alphas(pfv_ctx* h, int nalpha, const double* alpha_k33n) {
  return guarded(h, [&] {
    require(h->have_grid, "pfv_set_grid must be called first");
    require(nalpha >= 0 && nalpha <= 8 && (nalpha == 0 || alpha_k33n), "bad coupling tensors");
    const bool layout_change = (nalpha > 0) != (h->biot_nalpha > 0) || nalpha != h->biot_nalpha;
    h->biot_nalpha = nalpha;
    if (nalpha > 0) upload(h->biot_alpha, alpha_k33n, (size_t)nalpha * 9 * (size_t)h->nc, h->stream);
    if (layout_change) {
      h->have_mpsa_symbolic = false;  // LDS sizing of the node kernel depends on it
      h->have_biot_symbolic = false;
      h->biot_rows_complete = false;
    }
    h->have_biot_numeric = false;
  });
}

pfv_status pfv_biot_discretize(pfv_ctx* h, uint32_t flags) {
  return guarded(h, [&] {
    require(h->have_grid && h->have_mpsa_params, "grid and MPSA parameters must be set before discretize");
    require(h->biot_nalpha > 0, "pfv_biot_set_alphas first");
    auto s = h->stream;
    pfv::Timer tm;
    if (!h->have_topology || !h->have_symbolic || (flags & PFV_DISCR_REBUILD_TOPOLOGY)) {
      tm.start(s);
      pfv::build_topology(*h);
      h->stats.topology_ms = tm.stop(s);
      tm.start(s);
      pfv::build_symbolic(*h);
      h->stats.symbolic_ms = tm.stop(s);
      h->tpfa_mode = false;
      h->have_mpsa_symbolic = h->have_biot_symbolic = false;
      h->have_numeric = h->have_system = false;
    }
    if (!h->have_mpsa_symbolic) {
      pfv::mpsa_symbolic(*h);
      h->have_biot_symbolic = false;
    }
    if (!h->have_biot_symbolic) pfv::biot_symbolic(*h);
    tm.start(s);
    pfv::mpsa_run_node_kernel(*h);
    h->stats.node_ms = tm.stop(s);
    tm.start(s);
    pfv::mpsa_run_face_kernel(*h);
    for (int ka = 0; ka < h->biot_nalpha; ++ka) {
      pfv::biot_run_face_kernel(*h, ka);
      pfv::biot_run_cell_kernel(*h, ka);
    }
    h->stats.face_ms = tm.stop(s);
    h->have_mpsa_numeric = true;
    h->rows_complete_m = true;
    h->have_biot_numeric = true;
    h->biot_rows_complete = true;
    h->have_mech_system = false;
    h->filled[PFV_MAT_MECH_SYSTEM] = false;
  });
}

pfv_status pfv_biot_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces, const int32_t* faces,
                                     int64_t n_cells, const int32_t* cells, int keep_other_rows) {
  if (!h) return PFV_ERR_ARGUMENT;
  if (keep_other_rows && !h->biot_rows_complete) {
    h->err = "update of coupling terms that were never computed on this handle";
    return PFV_ERR_ARGUMENT;
  }
  if (h->biot_nalpha <= 0) {
    h->err = "pfv_biot_set_alphas first";
    return PFV_ERR_ARGUMENT;
  }
  // interaction regions of the faces' nodes (with the Biot tail) and the four MPSA matrices
  pfv_status st = pfv_mpsa_discretize_faces(h, flags, n_faces, faces, keep_other_rows);
  if (st != PFV_OK) return st;
  return guarded(h, [&] {
    require(n_cells >= 0 && (n_cells == 0 || cells), "bad cell list");
    for (int64_t i = 0; i < n_cells; ++i) require(cells[i] >= 0 && cells[i] < h->nc, "cell index out of range");
    auto s = h->stream;
    int32_t* csub = h->cell_subset.ensure(std::max<int64_t>(n_cells, 1));
    pfv::be_h2d(csub, cells, sizeof(int32_t) * (size_t)n_cells, s);
    if (!keep_other_rows) {
      for (int term = 0; term < PFV_BIOT_NUM_TERMS; ++term) {
        const int64_t nnz = pfv::biot_pattern(*h, term).nnz;
        for (int ka = 0; ka < h->biot_nalpha; ++ka) {
          double* v = h->biot_val[(size_t)term * h->biot_nalpha + ka].ensure(std::max<int64_t>(nnz, 1));
          pfv::be_memset(v, 0, sizeof(double) * (size_t)nnz, s);
        }
      }
    }
    for (int ka = 0; ka < h->biot_nalpha; ++ka) {
      if (n_faces > 0) pfv::biot_run_face_kernel(*h, ka, h->face_subset.p, n_faces);
      if (n_cells > 0) pfv::biot_run_cell_kernel(*h, ka, csub, n_cells);
    }
    if (!keep_other_rows) h->biot_rows_complete = false;
    h->have_biot_numeric = true;
  });
}

pfv_status pfv_biot_matrix_info(pfv_ctx* h, int term, int64_t* nrows, int64_t* ncols, int64_t* nnz) {
  return guarded(h, [&] {
    require(term >= 0 && term < PFV_BIOT_NUM_TERMS, "bad term");
    require(h->have_biot_symbolic, "pfv_biot_discretize first");
    const pfv::CsrPattern& P = pfv::biot_pattern(*h, term);
    if (nrows) *nrows = P.nrows;
    if (ncols) *ncols = P.ncols;
    if (nnz) *nnz = P.nnz;
  });
}

pfv_status pfv_biot_get_matrix(pfv_ctx* h, int term, int key, int32_t* indptr, int32_t* indices, double* data) {
  return guarded(h, [&] {
    require(term >= 0 && term < PFV_BIOT_NUM_TERMS, "bad term");
    require(h->have_biot_symbolic, "pfv_biot_discretize first");
    require(key >= 0 && key < h->biot_nalpha, "bad coupling key");
    const pfv::CsrPattern& P = pfv::biot_pattern(*h, term);
    auto s = h->stream;
    if (indptr) be_d2h(indptr, P.indptr.p, sizeof(int32_t) * (size_t)(P.nrows + 1), s);
    if (indices) be_d2h(indices, P.indices.p, sizeof(int32_t) * (size_t)P.nnz, s);
    if (data) {
      require(h->have_biot_numeric, "pfv_biot_discretize first");
      be_d2h(data, h->biot_val[(size_t)term * h->biot_nalpha + key].p, sizeof(double) * (size_t)P.nnz, s);
    }
  });
}

pfv_status pfv_mpsa_assemble(pfv_ctx* h, const double* bc_values, const double* source) {
  return guarded(h, [&] {
    require(h->have_mpsa_numeric, "pfv_mpsa_discretize first");
    require(!h->mpsa_subface_bc, "stress has sub-face rows (conditions per sub-face): collapse it before assembling");
    require(bc_values != nullptr, "bc_values is required");
    auto s = h->stream;
    const size_t nfd = (size_t)h->nf * h->nd, ncd = (size_t)h->nc * h->nd;
    double* in = h->vec_in.ensure(nfd + ncd);
    vec_in(h, in, bc_values, nfd);
    double* d_src = nullptr;
    if (source) {
      d_src = in + nfd;
      vec_in(h, d_src, source, ncd);
    }
    pfv::Timer tm;
    tm.start(s);
    if (!h->have_mech_system) {
      pfv::mpsa_assemble_system(*h);
      values_changed(h, Windows::drop);
    }
    pfv::mpsa_assemble_rhs(*h, in, d_src);
    h->stats.assemble_ms = tm.stop(s);
    h->have_mech_system = true;
    activate(h, h->pat_Am, h->val[PFV_MAT_MECH_SYSTEM].p, h->diag_m.p, h->rhs_m.p, h->nc * h->nd, h->nd, true);
  });
}

pfv_status pfv_device_memory(pfv_ctx* h, int64_t* free_bytes, int64_t* total_bytes) {
  return guarded(h, [&] {
    require(free_bytes && total_bytes, "null output");
#ifdef PFV_EMULATE
    *free_bytes = *total_bytes = -1;  // host emulation: unknown
#else
    size_t f = 0, t = 0;
    PFV_HIP_CHECK(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f + (int64_t)h->pool.cached;  // blocks parked in the handle's cache are reusable
    *total_bytes = (int64_t)t;
#endif
  });
}

pfv_status pfv_host_alloc(size_t bytes, void** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  if (bytes == 0) bytes = 8;
#ifdef PFV_EMULATE
  *out = std::malloc(bytes);
  return *out ? PFV_OK : PFV_ERR_HIP;
#else
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? PFV_OK : PFV_ERR_HIP;
#endif
}

void pfv_host_free(void* p) {
  if (!p) return;
#ifdef PFV_EMULATE
  std::free(p);
#else
  (void)hipHostFree(p);
#endif
}

pfv_status pfv_active_size(pfv_ctx* h, int64_t* n) {
  return guarded(h, [&] {
    require(n != nullptr, "null output");
    *n = h->active.valid ? h->active.n : 0;
  });
}

pfv_status pfv_get_rhs(pfv_ctx* h, double* b) {
  return guarded(h, [&] {
    require(h->active.valid && b, "assemble first");
    be_d2h(b, h->active.rhs, sizeof(double) * (size_t)h->active.n, h->stream);
  });
}

pfv_status pfv_spmv(pfv_ctx* h, int which, const double* x, double* y) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS && x && y, "bad argument");
    require((h->have_symbolic || which == PFV_MAT_USER_SYSTEM || which >= PFV_MAT_UPWIND) && h->filled[which],
            "matrix values have not been computed");
    const bool vs = which == PFV_MAT_VECTOR_SOURCE || which == PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE;
    if (!(vs && h->vs_implicit)) materialize_pattern(h, which);
    const pfv::CsrPattern& P = h->pattern_of(which);
    auto s = h->stream;
    pfv::Buf<double> dx, dy;
    dx.ensure((size_t)P.ncols);
    dy.ensure((size_t)P.nrows);
    be_h2d(dx.p, x, sizeof(double) * (size_t)P.ncols, s);
    if (vs && h->vs_implicit) pfv::spmv_vs_implicit(*h, h->val[which], dx.p, dy.p);
    else pfv::spmv(*h, P, h->val[which], dx.p, dy.p);
    be_d2h(y, dy.p, sizeof(double) * (size_t)P.nrows, s);
  });
}

pfv_status pfv_spmv_device(pfv_ctx* h, int which, const double* d_x, double* d_y) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS && d_x && d_y, "bad argument");
    require((h->have_symbolic || which == PFV_MAT_USER_SYSTEM || which >= PFV_MAT_UPWIND) && h->filled[which],
            "matrix values have not been computed");
    if ((which == PFV_MAT_VECTOR_SOURCE || which == PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE) && h->vs_implicit) {
      pfv::spmv_vs_implicit(*h, h->val[which], d_x, d_y);
      return;
    }
    materialize_pattern(h, which);
    pfv::spmv(*h, h->pattern_of(which), h->val[which], d_x, d_y);
  });
}

pfv_status pfv_spmv_device_rows(pfv_ctx* h, int which, int64_t nrows, const double* d_x, double* d_y) {
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS && d_x && d_y, "bad argument");
    require((h->have_symbolic || which == PFV_MAT_USER_SYSTEM || which >= PFV_MAT_UPWIND) && h->filled[which],
            "matrix values have not been computed");
    materialize_pattern(h, which);
    const pfv::CsrPattern& P = h->pattern_of(which);
    require(nrows >= 0 && nrows <= P.nrows, "nrows out of range");
    pfv::CsrPattern V;  // view of the leading rows (shares the index arrays)
    V.nrows = nrows;
    V.ncols = P.ncols;
    V.nnz = P.nrows ? (int64_t)((double)P.nnz * (double)nrows / (double)P.nrows) : 0;
    V.indptr.p = P.indptr.p;
    V.indices.p = P.indices.p;
    try {
      const bool sysmat = which == PFV_MAT_SYSTEM || which == PFV_MAT_MECH_SYSTEM || which == PFV_MAT_USER_SYSTEM;
      bool done = false;
      if (sysmat && nrows > 0 && P.nnz >= pfv::env_int("PFV_SPMV_WINDOW_MIN_NNZ", 20000)) {
        // the sharded Krylov loop's product with the owned rows: windowed kernel, window kept until
        // the matrix is assembled again
        if (h->win_rows_for != P.indices.p || h->win_rows_n != nrows) {
          V.nnz = P.nnz;  // (lidx is indexed by entry position)
          h->win_rows_checksum = 0;
          pfv::win_build(*h, V, h->win_rows);
          h->win_rows_for = P.indices.p;
          h->win_rows_n = nrows;
        }
        if (h->win_rows.ok) {
          pfv::LinSys sys;
          sys.P = &V;
          sys.val = h->val[which].p;
          sys.win = &h->win_rows;
          pfv::sys_spmv(*h, sys, d_x, d_y);
          done = true;
        }
      }
      if (!done) pfv::spmv(*h, V, h->val[which], d_x, d_y);
    } catch (...) {
      V.indptr.p = nullptr;
      V.indices.p = nullptr;
      throw;
    }
    V.indptr.p = nullptr;  // not owned
    V.indices.p = nullptr;
  });
}

pfv_status pfv_copy_device_vector(pfv_ctx* h, int which, double* d_dst, int64_t count) {
  return guarded(h, [&] {
    require(h->active.valid && d_dst && count >= 0 && count <= h->active.n, "bad argument / assemble first");
    require(which == 0 || which == 1, "which must be 0 (rhs) or 1 (diagonal)");
    pfv::be_d2d(d_dst, which == 0 ? h->active.rhs : h->active.diag, sizeof(double) * (size_t)count, h->stream);
  });
}

pfv_status pfv_set_stream(pfv_ctx* h, void* hip_stream) {
  return guarded(h, [&] {
#ifdef PFV_EMULATE
    (void)hip_stream;
#else
    pfv::be_sync(h->stream);
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = the legacy default stream
#endif
  });
}

pfv_status pfv_reset_stream(pfv_ctx* h) {
  return guarded(h, [&] {
#ifndef PFV_EMULATE
    pfv::be_sync(h->stream);
    h->stream = h->own_stream;
#endif
  });
}

pfv_status pfv_get_device_rhs(pfv_ctx* h, double** d_b, double** d_diag) {
  return guarded(h, [&] {
    require(h->have_system && h->have_flow_rhs, "assemble first");
    if (d_b) *d_b = h->rhs.p;
    if (d_diag) *d_diag = h->diag.p;
  });
}

pfv_status pfv_sync(pfv_ctx* h) {
  return guarded(h, [&] { pfv::be_sync(h->stream); });
}

// The tail of pfv_set_system and pfv_csr_set_system: pat_user, val[PFV_MAT_USER_SYSTEM] and rhs_u hold the system.
// Extracts the diagonal, refuses a column out of range or a zero diagonal, and makes the system the active one.
static void user_system_ready(pfv_ctx* h) {
  auto s = h->stream;
  pfv::CsrPattern& P = h->pat_user;
  const int64_t n = P.nrows;
  const int32_t* ip = P.indptr.p;
  const int32_t* ix = P.indices.p;
  double* v = h->val[PFV_MAT_USER_SYSTEM].p;
  double* dg = h->diag_u.ensure(n);
  int32_t* st = h->status.ensure(16);
  pfv::be_memset(st, 0, sizeof(int32_t) * 4, s);
  pfv::parallel_for(s, n, PFV_LAMBDA(int64_t i) {
    double d = 0.0;
    bool bad = false;
    for (int e = ip[i]; e < ip[i + 1]; ++e) {
      const int cidx = ix[e];
      if (cidx < 0 || cidx >= n) bad = true;
      else if (cidx == i) d += v[e];
    }
    dg[i] = d;
    if (bad) pfv::atomic_max_i32(st + 1, 1);
    if (!(d != 0.0) || !(d == d)) pfv::atomic_max_i32(st + 0, (int32_t)(i < 0x7fffffff ? i + 1 : 0x7fffffff));
  });
  int32_t sth[2];
  be_d2h(sth, st, sizeof(sth), s);
  require(!sth[1], "column index out of range");
  if (sth[0])
    throw pfv::Error(PFV_ERR_UNSUPPORTED, "zero diagonal entry in row " + std::to_string(sth[0] - 1) +
                                              ": the Jacobi-preconditioned solver does not apply");
  h->filled[PFV_MAT_USER_SYSTEM] = true;
  values_changed(h, Windows::drop);  // (the user-system buffers are reused: same pointers, new matrix)
  activate(h, P, v, dg, h->rhs_u.p, n, 1, false);
}

pfv_status pfv_set_system(pfv_ctx* h, int64_t n, const int32_t* indptr, const int32_t* indices,
                          const double* data, const double* rhs) {
  return guarded(h, [&] {
    require(n > 0 && indptr && indices && data && rhs, "bad system");
    require(indptr[0] == 0, "indptr must start at 0");
    const int64_t nnz = indptr[n];
    require(nnz >= 0, "bad indptr");
    auto s = h->stream;
    pfv::CsrPattern& P = h->pat_user;
    P.nrows = P.ncols = n;
    P.nnz = nnz;
    int32_t* ip = P.indptr.ensure(n + 1);
    int32_t* ix = P.indices.ensure(std::max<int64_t>(nnz, 1));
    double* v = h->val[PFV_MAT_USER_SYSTEM].ensure(std::max<int64_t>(nnz, 1));
    double* b = h->rhs_u.ensure(n);
    be_h2d(ip, indptr, sizeof(int32_t) * (size_t)(n + 1), s);
    be_h2d(ix, indices, sizeof(int32_t) * (size_t)nnz, s);
    be_h2d(v, data, sizeof(double) * (size_t)nnz, s);
    be_h2d(b, rhs, sizeof(double) * (size_t)n, s);
    int mr = 0;
    for (int64_t i = 0; i < n; ++i) mr = std::max(mr, indptr[i + 1] - indptr[i]);
    P.max_row = mr;
    user_system_ready(h);
  });
}

pfv_status pfv_amg_setup(pfv_ctx* h, int64_t n_own) {
  return guarded(h, [&] {
    if (h->precond == PFV_PRECOND_SWEEP)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_SWEEP has no AMG hierarchy and no sharded form");
    if (h->precond == PFV_PRECOND_AMG_NNS)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_AMG_NNS has no sharded form: pfv_set_preconditioner(PFV_PRECOND_AMG) "
                                            "or PFV_PRECOND_JACOBI for sharded solves");
    require(h->active.valid, "assemble first");
    const int bs = h->active_bs;
    const int64_t n = h->active.n;
    if (n_own <= 0) n_own = n;
    require(n_own <= n && n_own % bs == 0, "bad block size");
    auto s = h->stream;
    if (!h->amg_block) h->amg_block = std::make_unique<pfv::Amg>();
    h->amg_block->valid = false;
    h->amg_block->dist.reset();  // (a coupled hierarchy of an earlier pfv_amg_setup_sharded)
    const pfv::CsrPattern* P = h->active.P;
    const double* val = h->active.val;
    if (n_own < n) {
      // leading block: drop the columns >= n_own (halo cells of the subdomain)
      const int32_t* ip = P->indptr;
      const int32_t* ix = P->indices;
      pfv::Buf<int32_t> len;
      pfv::Buf<int64_t> pos;
      int32_t* ln = len.ensure(n_own + 1);
      int64_t* ps = pos.ensure(n_own + 1);
      pfv::parallel_for(s, n_own, PFV_LAMBDA(int64_t r) {
        int m = 0;
        for (int e = ip[r]; e < ip[r + 1]; ++e) m += ix[e] < n_own ? 1 : 0;
        ln[r] = m;
      });
      pfv::exclusive_scan<int32_t, int64_t>(s, h->scratch, ln, ps, (size_t)n_own);
      const int64_t nnz = pfv::read_scalar<int64_t>(s, ps + n_own);
      pfv::CsrPattern& B = h->pat_block;
      B.nrows = B.ncols = n_own;
      B.nnz = nnz;
      B.max_row = P->max_row;
      int32_t* bp = B.indptr.ensure(n_own + 1);
      int32_t* bx = B.indices.ensure(std::max<int64_t>(nnz, 1));
      double* bv = h->val_block.ensure(std::max<int64_t>(nnz, 1));
      pfv::parallel_for(s, n_own + 1, PFV_LAMBDA(int64_t r) {
        bp[r] = (int32_t)ps[r];
        if (r < n_own) {
          int64_t o = ps[r];
          for (int e = ip[r]; e < ip[r + 1]; ++e)
            if (ix[e] < n_own) {
              bx[o] = ix[e];
              bv[o] = val[e];
              ++o;
            }
        }
      });
      P = &B;
      val = bv;
    }
    const pfv::WinCsr* bw = nullptr;
    if (P->nnz >= pfv::env_int("PFV_SPMV_WINDOW_MIN_NNZ", 20000)) {
      pfv::win_build(*h, *P, h->win_block);
      bw = &h->win_block;
    }
    pfv::amg_setup(*h, *h->amg_block, *P, val, bs, h->active.diag, bw);  // the leading block keeps its diagonal
    amg_setup_stats(h, *h->amg_block, (int64_t)h->amg_block->nlev, h->amg_block->lev[h->amg_block->nlev - 1]->n, h->amg_block->reused);
    h->amg_last = 2;
  });
}

pfv_status pfv_amg_setup_sharded(pfv_ctx* h, int64_t n_own, const pfv_shard_hooks* hooks, int rank, int world,
                                 int n_peers, const int32_t* peers, const int64_t* send_ptr,
                                 const int32_t* send_idx, const int64_t* recv_ptr, const int32_t* recv_pos) {
  return guarded(h, [&] {
    if (h->precond == PFV_PRECOND_SWEEP)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_SWEEP has no AMG hierarchy and no sharded form");
    if (h->precond == PFV_PRECOND_AMG_NNS)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_AMG_NNS has no sharded form: pfv_set_preconditioner(PFV_PRECOND_AMG) "
                                            "or PFV_PRECOND_JACOBI for sharded solves");
    require(h->active.valid, "assemble first");
    const int bs = h->active_bs;
    const int64_t n = h->active.n;
    require(n_own > 0 && n_own <= n && n_own % bs == 0 && n % bs == 0, "n_own out of range");
    require(hooks && hooks->sendrecv && hooks->allgather, "the sendrecv and allgather hooks are required");
    require(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    require(n_peers >= 0 && (n_peers == 0 || (peers && send_ptr && recv_ptr)), "bad halo plan");
    const int64_t own_cells = n_own / bs, loc_cells = n / bs;
    auto plan = std::make_unique<pfv::AmgPlan>();
    plan->n_peers = n_peers;
    plan->peers.assign(peers, peers + n_peers);
    plan->send_ptr.assign(1, 0);
    plan->recv_ptr.assign(1, 0);
    if (n_peers > 0) {
      plan->send_ptr.assign(send_ptr, send_ptr + n_peers + 1);
      plan->recv_ptr.assign(recv_ptr, recv_ptr + n_peers + 1);
    }
    require(plan->send_ptr.front() == 0 && plan->recv_ptr.front() == 0, "halo plan: offsets must start at 0");
    for (int p = 0; p < n_peers; ++p) {
      require(plan->send_ptr[p + 1] >= plan->send_ptr[p] && plan->recv_ptr[p + 1] >= plan->recv_ptr[p],
              "halo plan: offsets must be non-decreasing");
      require(peers[p] >= 0 && peers[p] < world && peers[p] != rank, "peer out of range");
    }
    const int64_t ns = plan->send_ptr.back(), nr = plan->recv_ptr.back();
    require((ns == 0 || send_idx) && (nr == 0 || recv_pos), "halo plan: index lists missing");
    for (int64_t k = 0; k < ns; ++k) require(send_idx[k] >= 0 && send_idx[k] < own_cells, "halo plan: send index is not an owned cell");
    for (int64_t k = 0; k < nr; ++k)
      require(recv_pos[k] >= own_cells && recv_pos[k] < loc_cells, "halo plan: receive position is not a halo cell");
    require(nr == loc_cells - own_cells, "halo plan: every halo cell must be received exactly once");
    plan->h_send_idx.assign(send_idx, send_idx + ns);
    plan->h_recv_pos.assign(recv_pos, recv_pos + nr);
    plan->n_own = own_cells;
    plan->n_halo = loc_cells - own_cells;
    pfv::amg_plan_upload(*h, *plan);
    if (!h->amg_block) h->amg_block = std::make_unique<pfv::Amg>();
    pfv::Amg& amg = *h->amg_block;
    amg.valid = false;
    if (!amg.dist) amg.dist = std::make_unique<pfv::AmgDist>();
    amg.dist->hooks = *hooks;
    amg.dist->rank = rank;
    amg.dist->world = world;
    amg.dist->plan.clear();
    amg.dist->plan.push_back(std::move(plan));
    // the rows of the owned unknowns over all local columns (owned + halo)
    const pfv::CsrPattern& P = *h->active.P;
    pfv::CsrPattern& V = amg.dist->rows0;  // (borrows the index arrays: see ~AmgDist)
    V.nrows = n_own;
    V.ncols = n;
    V.nnz = P.nnz;
    V.max_row = P.max_row;
    V.indptr.p = P.indptr.p;
    V.indices.p = P.indices.p;
    // the windows of the owned rows (built beside the face kernel, or by the previous sharded solve): the windows of the
    // strength-filtered operator are derived from them instead of hashed and sorted from scratch (spmv_win.inc: win_derive)
    const pfv::WinCsr* win0 = (bs == 1 && h->win_rows.ok && h->win_rows_for == P.indices.p && h->win_rows_n == n_own &&
                               h->win_rows.nrows == n_own && pfv::env_int("PFV_SHARD_WIN0", 1) != 0)
                                  ? &h->win_rows
                                  : nullptr;
    pfv::amg_setup(*h, amg, V, h->active.val, bs, nullptr, win0);
    amg_setup_stats(h, amg, (int64_t)(amg.nlev + (amg.dist->glob ? amg.dist->glob->nlev - 1 : 0)), amg.dist->gN, amg.reused);
  });
}

pfv_status pfv_amg_apply_device(pfv_ctx* h, const double* d_r, double* d_z) {
  return guarded(h, [&] {
    require(h->amg_block && h->amg_block->valid, "pfv_amg_setup first");
    require(d_r && d_z && d_r != d_z, "bad vectors");
    if (h->amg_block->dist) pfv::amg_apply_dist(*h, *h->amg_block, d_r, d_z);
    else pfv::amg_cycle(*h, *h->amg_block, 0, d_r, d_z);
  });
}

pfv_status pfv_set_preconditioner(pfv_ctx* h, int kind) {
  return guarded(h, [&] {
    require(kind == PFV_PRECOND_JACOBI || kind == PFV_PRECOND_AMG || (kind == PFV_PRECOND_BLOCK && h->block_pc) ||
                (kind == PFV_PRECOND_AMG_NNS && h->nns_k > 0) || kind == PFV_PRECOND_SWEEP,
            "unknown preconditioner (PFV_PRECOND_BLOCK: pfv_set_block_preconditioner first; PFV_PRECOND_AMG_NNS: "
            "pfv_set_near_null_space first)");
    h->precond = kind;
  });
}

pfv_status pfv_set_block_preconditioner(pfv_ctx* h, int64_t n_blocks, const int64_t* block_ptr, int gauss_seidel) {
  return guarded(h, [&] {
    require(n_blocks >= 1 && block_ptr != nullptr && block_ptr[0] == 0, "bad block layout");
    for (int64_t k = 0; k < n_blocks; ++k) require(block_ptr[k + 1] > block_ptr[k], "blocks must be non-empty and ascending");
    if (!h->block_pc) h->block_pc = std::make_unique<pfv::BlockPc>();
    h->block_pc->ptr.assign(block_ptr, block_ptr + n_blocks + 1);
    h->block_pc->gs = gauss_seidel != 0;
    h->block_pc->for_val = nullptr;
    h->precond = PFV_PRECOND_BLOCK;
  });
}

pfv_status pfv_set_near_null_space(pfv_ctx* h, int bs, int k, const double* B) {
  return guarded(h, [&] {
    require(h->active.valid, "assemble first");
    require(k >= 0, "k must not be negative");
    if (k > pfv::kNnsMaxModes) throw pfv::Error(PFV_ERR_UNSUPPORTED, "near-null space: at most 8 modes");
    const int64_t n = h->active.n;
    if (k == 0) {
      h->nns_k = h->nns_bs = 0;
      h->nns_n = 0;
      h->nns_B.clear();
      h->nns_key = 0;
      if (h->precond == PFV_PRECOND_AMG_NNS) h->precond = PFV_PRECOND_JACOBI;
      return;
    }
    require(bs >= 1 && bs <= pfv::kNnsMaxModes && n % bs == 0, "near-null space: bad block size");
    unsigned long long key = 1469598103934665603ull;  // FNV-1a over what the modes are made of
    auto mix = [&key](const void* p, size_t bytes) {
      const unsigned char* c = static_cast<const unsigned char*>(p);
      for (size_t q = 0; q < bytes; ++q) key = (key ^ c[q]) * 1099511628211ull;
    };
    mix(&k, sizeof k);
    mix(&bs, sizeof bs);
    mix(&n, sizeof n);
    if (B == nullptr) {
      require(h->active_is_grid && h->nd >= 2 && bs == h->nd && h->active_bs == h->nd && n == h->nc * h->nd,
              "near-null space B == NULL: rigid-body modes of the grid need the assembled mechanics system (bs = nd)");
      require(k == (h->nd == 2 ? 3 : 6), "near-null space B == NULL: k must be 3 in 2-D, 6 in 3-D");
      h->nns_B.clear();
      const unsigned long long tag = 0x67726964ull;  // device-made: the grid the centres belong to
      mix(&tag, sizeof tag);
      mix(&h->grid_serial, sizeof h->grid_serial);
    } else {
      h->nns_B.assign(B, B + (size_t)n * k);
      mix(B, sizeof(double) * (size_t)n * k);
    }
    h->nns_k = k;
    h->nns_bs = bs;
    h->nns_n = n;
    h->nns_key = key;
  });
}

// the near-null space in the numbering of the system the Krylov loop works on, row-major [n][k]
static const double* nns_modes(pfv_ctx* h, bool permuted) {
  auto s = h->stream;
  const int64_t n = h->nns_n;
  const int k = h->nns_k, bs = h->nns_bs;
  double* col = h->nns_col.ensure((size_t)(n * k));
  if (h->nns_B.empty()) pfv::nns_rigid_body_modes(*h, h->nd, h->nc, h->ccen, col);
  else pfv::be_h2d(col, h->nns_B.data(), sizeof(double) * (size_t)(n * k), s);
  double* tmp = h->nns_row.ensure((size_t)(n * k));
  const double* src = col;
  if (permuted) {  // the renumbering of the system (reorder.inc), column by column
    for (int j = 0; j < k; ++j) pfv::permute_vector(*h, n, bs, col + (size_t)j * n, tmp + (size_t)j * n, true);
    pfv::be_d2d(col, tmp, sizeof(double) * (size_t)(n * k), s);
  }
  pfv::parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    for (int j = 0; j < k; ++j) tmp[r * k + j] = src[(int64_t)j * n + r];
  });
  return tmp;
}

// the cell centres in the numbering of the system (device-made modes only; nullptr for the caller's modes)
static const double* nns_centres(pfv_ctx* h, bool permuted) {
  if (!h->nns_B.empty()) return nullptr;
  const int64_t nc = h->nc;
  double* cc = h->nns_cc.ensure((size_t)(3 * nc));
  for (int d = 0; d < 3; ++d) {
    if (permuted) pfv::permute_vector(*h, nc, 1, h->ccen.p + d * nc, cc + d * nc, true);
    else pfv::be_d2d(cc + d * nc, h->ccen.p + d * nc, sizeof(double) * (size_t)nc, h->stream);
  }
  return cc;
}

pfv_status pfv_amg_nns_level(pfv_ctx* h, int level, int64_t* info, int32_t* agg, double* P, double* B, double* Bc,
                             int32_t* indptr, int32_t* indices, double* val) {
  return guarded(h, [&] {
    require(info != nullptr, "info is required");
    require(h->amg_nns && h->amg_nns->valid, "no near-null-space hierarchy (solve with PFV_PRECOND_AMG_NNS first)");
    pfv::AmgNns& H = *h->amg_nns;
    require(level >= 0 && (size_t)level < H.nlev, "level out of range");
    const pfv::NnsLevel& L = *H.lev[(size_t)level];
    const int k = H.k;
    info[0] = L.n;
    info[1] = L.bs;
    info[2] = k;
    info[3] = L.nagg;
    info[4] = L.P->nnz;
    info[5] = (int64_t)H.nlev;
    auto s = h->stream;
    if (agg && L.nagg > 0) be_d2h(agg, L.agg.p, sizeof(int32_t) * (size_t)L.cells, s);
    if (P && L.nagg > 0) be_d2h(P, L.Pt.p, sizeof(double) * (size_t)(L.n * k), s);
    if (B) be_d2h(B, L.B.p, sizeof(double) * (size_t)(L.n * k), s);
    if (Bc && L.nagg > 0) be_d2h(Bc, L.Bc.p, sizeof(double) * (size_t)(L.nagg * k * k), s);
    if (indptr) be_d2h(indptr, L.P->indptr.p, sizeof(int32_t) * (size_t)(L.n + 1), s);
    if (indices) be_d2h(indices, L.P->indices.p, sizeof(int32_t) * (size_t)L.P->nnz, s);
    if (val) be_d2h(val, L.val, sizeof(double) * (size_t)L.P->nnz, s);
    pfv::be_sync(s);
  });
}

pfv_status pfv_amg_nns_apply_device(pfv_ctx* h, const double* d_r, double* d_z) {
  return guarded(h, [&] {
    require(h->amg_nns && h->amg_nns->valid, "no near-null-space hierarchy (solve with PFV_PRECOND_AMG_NNS first)");
    require(d_r && d_z && d_r != d_z, "bad vectors");
    pfv::amg_nns_cycle(*h, *h->amg_nns, 0, d_r, d_z);
  });
}

pfv_status pfv_amg_level(pfv_ctx* h, int level, int64_t* info, double* params, int32_t* sys_indptr, int32_t* sys_indices,
                         double* sys_val, int32_t* a_indptr, int32_t* a_indices, double* a_val, int32_t* op_indptr,
                         int32_t* op_indices, double* op_val, double* dinv, int32_t* agg, int32_t* mptr, int32_t* mem,
                         double* dense) {
  return guarded(h, [&] {
    require(info != nullptr, "info is required");
    const pfv::Amg* ap = h->amg_last == 1 ? h->amg.get() : (h->amg_last == 2 ? h->amg_block.get() : nullptr);
    require(ap && ap->valid, "no AMG hierarchy (pfv_amg_setup or a solve with PFV_PRECOND_AMG first)");
    const pfv::Amg& amg = *ap;
    if (amg.dist) throw pfv::Error(PFV_ERR_UNSUPPORTED, "pfv_amg_level does not read the coupled hierarchy of a sharded solve");
    require(level >= 0 && (size_t)level < amg.nlev, "level out of range");
    const size_t l = (size_t)level;
    const pfv::AmgLevel& L = *amg.lev[l];
    const bool last = l + 1 == amg.nlev;
    // the matrix the level was coarsened from: the strength-filtered copy on level 0 when the filter is on
    const bool filtered = l == 0 && amg.filter_theta > 0.0 && amg.filt_nnz > 0;
    const pfv::CsrPattern* Pa = filtered ? &amg.filtP : L.P;
    const double* Va = filtered ? amg.filtV.p : L.val;
    const pfv::AmgPath path = pfv::amg_level_path(amg, l);
    int maxcap = 0;
    for (const auto& g : amg.gal_sizes) maxcap = std::max(maxcap, g.maxcap);
    info[0] = L.n;
    info[1] = amg.bs;
    info[2] = (int64_t)amg.nlev;
    info[3] = last ? 0 : L.nc_cells;
    info[4] = Pa->nnz;
    info[5] = L.P->nnz;
    info[6] = l == 0 ? amg.sysP->nnz : 0;
    info[7] = L.v32 ? 1 : 0;
    info[8] = (path.small ? 1 : 0) | (path.fuse_up ? 2 : 0) | (path.fuse_big ? 4 : 0) | (path.twice ? 8 : 0) |
              (path.second ? 16 : 0) | (path.second && amg.fuse_cycle ? 32 : 0) | (last && amg.dense_ok ? 64 : 0) |
              (last && !amg.dense_ok ? 128 : 0);
    info[9] = amg.dense_ok ? 1 : 0;
    info[10] = amg.gamma;
    info[11] = amg.gamma_levels;
    info[12] = amg.fuse_rows;
    info[13] = amg.fuse_cycle ? 1 : 0;
    info[14] = amg.reused ? 1 : 0;
    info[15] = amg.filter_level0 ? 1 : 0;
    info[16] = amg.restrict_lanes ? 1 : 0;
    info[17] = (L.win && L.win->ok) ? 1 : 0;
    info[18] = (!last && L.mptr.p && L.mem.p) ? 1 : 0;
    info[19] = maxcap;
    info[20] = pfv::kAmgDenseMax;
    info[21] = pfv::kGalEpl;
    info[22] = pfv::kGalMaxMembers;
    info[23] = pfv::kAmgWTopRows;
    if (params) {
      params[0] = L.omega;
      params[1] = amg.alpha;
      params[2] = amg.filter_theta;
      params[3] = L.rho;
    }
    auto s = h->stream;
    auto csr = [&](const pfv::CsrPattern& P, const double* v, int32_t* ip, int32_t* ix, double* val) {
      if (ip) be_d2h(ip, P.indptr.p, sizeof(int32_t) * (size_t)(P.nrows + 1), s);
      if (ix && P.nnz > 0) be_d2h(ix, P.indices.p, sizeof(int32_t) * (size_t)P.nnz, s);
      if (val && P.nnz > 0) be_d2h(val, v, sizeof(double) * (size_t)P.nnz, s);
    };
    if (l == 0) csr(*amg.sysP, amg.sysV, sys_indptr, sys_indices, sys_val);
    csr(*Pa, Va, a_indptr, a_indices, a_val);
    csr(*L.P, L.val, op_indptr, op_indices, op_val);
    if (dinv) be_d2h(dinv, L.dinv.p, sizeof(double) * (size_t)L.n, s);
    const int64_t cells = L.n / amg.bs;
    if (!last) {
      if (agg) be_d2h(agg, L.agg.p, sizeof(int32_t) * (size_t)cells, s);
      if (mptr) be_d2h(mptr, L.mptr.p, sizeof(int32_t) * (size_t)(L.nc_cells + 1), s);
      if (mem) be_d2h(mem, L.mem.p, sizeof(int32_t) * (size_t)cells, s);
    }
    if (dense && last && amg.dense_ok) be_d2h(dense, amg.dense.p, sizeof(double) * (size_t)(L.n * L.n), s);
    pfv::be_sync(s);
  });
}

pfv_status pfv_amg_level_rhs(pfv_ctx* h, int level, double* out) {
  return guarded(h, [&] {
    require(out != nullptr, "out is required");
    const pfv::Amg* ap = h->amg_last == 1 ? h->amg.get() : (h->amg_last == 2 ? h->amg_block.get() : nullptr);
    require(ap && ap->valid, "no AMG hierarchy (pfv_amg_setup or a solve with PFV_PRECOND_AMG first)");
    if (ap->dist) throw pfv::Error(PFV_ERR_UNSUPPORTED, "pfv_amg_level_rhs does not read the coupled hierarchy of a sharded solve");
    require(level >= 1 && (size_t)level < ap->nlev, "level out of range");
    const pfv::AmgLevel& L = *ap->lev[(size_t)level];
    require(L.b.p != nullptr, "the level has no right-hand side yet");
    be_d2h(out, L.b.p, sizeof(double) * (size_t)L.n, h->stream);
    pfv::be_sync(h->stream);
  });
}

// The system the Krylov loop works on: the active one, renumbered along the cell order when it is a
// grid system (reorder.inc), with the SpMV windows of its pattern (spmv_win.inc).  Copies and
// windows are kept until the matrix is assembled again.
static pfv::LinSys solver_system(pfv_ctx* h, bool& permuted) {
  pfv::LinSys sys = h->active;
  const int bs = h->active_bs;
  permuted = false;
  if (h->active_is_grid && sys.n == h->nc * bs && pfv::env_int("PFV_REORDER", 1) != 0 &&
      h->nc >= pfv::env_int("PFV_REORDER_MIN_CELLS", 256)) {
    if (!h->have_cell_order) pfv::build_cell_order(*h);
  }
  if (h->active_is_grid && h->have_cell_order && !h->cell_order_identity && sys.n == h->nc * bs &&
      pfv::env_int("PFV_REORDER", 1) != 0 && h->nc >= pfv::env_int("PFV_REORDER_MIN_CELLS", 256)) {
    if (h->perm_for_val != sys.val) {
      pfv::permute_matrix(*h, sys, bs);
      h->perm_for_val = sys.val;
      values_changed(h, Windows::drop, true);  // (the copy's buffers are shared by all grid systems)
    }
    pfv::permute_vector(*h, sys.n, bs, sys.rhs, h->rhs_perm.ensure(sys.n), true);
    sys.P = &h->pat_perm;
    sys.val = h->val_perm.p;
    sys.diag = h->diag_perm.p;
    sys.rhs = h->rhs_perm.p;
    permuted = true;
  }
  sys.win = nullptr;
  if (sys.P->nnz >= pfv::env_int("PFV_SPMV_WINDOW_MIN_NNZ", 20000)) {
    if (h->win_for != sys.P->indices.p || !h->win_sys.ok || pfv::env_int("PFV_SPMV_WINDOW", 1) == 0) {
      h->win_sys_checksum = 0;
      pfv::win_build(*h, *sys.P, h->win_sys);
      h->win_for = sys.P->indices.p;
      if (h->win_sys.ok && sys.P == &h->pat_A && h->have_symbolic) h->win_sys_checksum = h->pat_A_checksum;
    }
    sys.win = &h->win_sys;
  }
  return sys;
}

pfv_status pfv_solve(pfv_ctx* h, int method, double rtol, int maxit, int restart, const double* x0,
                     double* x, pfv_solve_info* info) {
  pfv::SolveResult res;
  pfv_status st = guarded(h, [&] {
    require(h->active.valid, "assemble first");
    require(x != nullptr, "x is required");
    require(method == PFV_SOLVE_CG || method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_CG, PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    const bool sweep_transport = h->precond == PFV_PRECOND_SWEEP && transport_is_active(h);
    const bool sweep_advdiff = h->precond == PFV_PRECOND_SWEEP && !sweep_transport && advdiff_is_active(h);
    if (h->precond == PFV_PRECOND_SWEEP && !sweep_transport && !sweep_advdiff)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_SWEEP applies to the transport system (pfv_upwind_assemble) and to "
                                            "the advection-diffusion system (pfv_advdiff_assemble) of the handle only: the "
                                            "active system is neither");
    h->stats.sweep_levels = h->stats.sweep_core_cells = h->stats.sweep_launches = 0;
    h->stats.sweep_direct_steps = h->stats.sweep_direct_fallbacks = 0;
    h->stats.sweep_order_ms = 0.0;
    if (h->precond == PFV_PRECOND_SWEEP) {
      // the flow order is a function of the flux alone: built by the first solve that needs it, before the system is judged
      const int which = sweep_transport ? PFV_MAT_TRANSPORT_SYSTEM : PFV_MAT_ADVDIFF_SYSTEM;
      if (!h->sweep) h->sweep = std::make_unique<pfv::Sweep>();
      if (!h->sweep->valid || h->sweep->for_system != which) {
        pfv::sweep_build_order(*h, *h->sweep, sweep_transport ? h->transport_q : h->adv_q.p, which);
        h->stats.sweep_order_ms = h->sweep->order_ms;
      }
    }
    if (transport_is_active(h) && h->transport_zero_diag >= 0)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "zero diagonal entry in row " + std::to_string(h->transport_zero_diag) +
                                                " of the transport system (a cell without outflow and without an "
                                                "accumulation term): the Jacobi-preconditioned solver does not apply");
    if (h->have_advdiff && active_is(h, PFV_MAT_ADVDIFF_SYSTEM) && h->advdiff_zero_diag >= 0)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "zero diagonal entry in row " + std::to_string(h->advdiff_zero_diag) +
                                                " of the advection-diffusion system: the solver does not apply");
    auto s = h->stream;
    const size_t n = (size_t)h->active.n;
    double* dx = h->xsol.ensure(n);
    if (x0) vec_in(h, dx, x0, n); else pfv::be_memset(dx, 0, n * sizeof(double), s);
    pfv::Timer tm;
    tm.start(s);
    bool permuted = false;
    const pfv::LinSys sys = solver_system(h, permuted);
    h->stats.solve_renumbered = permuted ? 1 : 0;
    double* dxs = dx;
    if (permuted) {
      dxs = h->x_perm.ensure(n);
      if (x0) pfv::permute_vector(*h, (int64_t)n, h->active_bs, dx, dxs, true);
      else pfv::be_memset(dxs, 0, n * sizeof(double), s);
    }
    pfv::Precond M;
    const pfv::Precond* Mp = nullptr;
    const long long launches_before_setup = pfv::launch_counter().load(std::memory_order_relaxed);
    if (h->precond == PFV_PRECOND_AMG) {
      if (!h->amg) h->amg = std::make_unique<pfv::Amg>();
      if (!h->amg->valid || h->amg_for_val != sys.val) {
        pfv::amg_setup(*h, *h->amg, *sys.P, sys.val, h->active_bs, sys.diag, sys.win);
        h->amg_for_val = sys.val;
        h->amg_last = 1;
        amg_setup_stats(h, *h->amg, (int64_t)h->amg->nlev, h->amg->lev[h->amg->nlev - 1]->n, h->amg->reused);
        h->stats.amg_stale_rematches = h->amg->stale_rematches;
        h->stats.amg_level0_nnz = h->amg->lev[0]->P->nnz;
        h->stats.amg_filter_theta = h->amg->filter_level0 ? h->amg->filter_theta : 0.0;
      }
      M.amg = h->amg.get();
      Mp = &M;
    } else if (h->precond == PFV_PRECOND_AMG_NNS) {
      require(h->nns_k > 0 && h->nns_n == (int64_t)n && (!permuted || h->nns_bs == h->active_bs),
              "the near-null space does not fit the active system (pfv_set_near_null_space again)");
      require(!h->nns_B.empty() || h->active_is_grid, "rigid-body modes of the grid need the assembled mechanics system");
      if (!h->amg_nns) h->amg_nns = std::make_unique<pfv::AmgNns>();
      const unsigned long long cfg = pfv::amg_nns_cfg(h->nns_bs);
      if (!h->amg_nns->valid || h->nns_stale || h->amg_nns_for_val != sys.val || h->amg_nns_key != h->nns_key ||
          h->amg_nns_cfg != cfg) {
        const double* B0 = nns_modes(h, permuted);
        pfv::amg_nns_setup(*h, *h->amg_nns, *sys.P, sys.val, h->nns_bs, h->nns_k, B0, nns_centres(h, permuted));
        h->amg_nns_for_val = sys.val;
        h->amg_nns_key = h->nns_key;
        h->amg_nns_cfg = cfg;
        h->nns_stale = false;
        const pfv::AmgNns& H = *h->amg_nns;
        amg_setup_stats(h, H, (int64_t)H.nlev, H.lev[H.nlev - 1]->n, false);
        h->stats.amg_level0_nnz = sys.P->nnz;
        h->stats.amg_filter_theta = 0.0;
        h->stats.amg_nns_modes = H.k;
      }
      M.nns = h->amg_nns.get();
      Mp = &M;
    } else if (h->precond == PFV_PRECOND_BLOCK) {
      require(h->block_pc && !permuted, "pfv_set_block_preconditioner first (user systems only)");
      require(h->block_pc->ptr.back() == (int64_t)n, "the block layout does not cover the system");
      if (h->block_pc->for_val != sys.val) {
        pfv::blockpc_setup(*h, *h->block_pc, *sys.P, sys.val);
        h->stats.amg_setup_ms = h->block_pc->setup_ms;
      }
      M.blocks = h->block_pc.get();
      M.P = sys.P;
      M.val = sys.val;
      M.diag = sys.diag;
      Mp = &M;
    } else if (h->precond == PFV_PRECOND_SWEEP) {
      pfv::Sweep& sw = *h->sweep;
      pfv::sweep_set_numbering(*h, sw, permuted);
      pfv::sweep_make_plan(sw);
      h->stats.sweep_levels = sw.nlev;
      h->stats.sweep_core_cells = sw.n_core;
      h->stats.sweep_launches = (int64_t)sw.plan.size();
      M.sweep = &sw;
      M.P = sys.P;
      M.val = sys.val;
      M.diag = sys.diag;
      Mp = &M;
    }
    const bool sweep_direct = M.sweep && sweep_transport && M.sweep->n_core == 0;
    const long long launches_before_loop = pfv::launch_counter().load(std::memory_order_relaxed);
    h->stats.amg_setup_launches = (int64_t)(launches_before_loop - launches_before_setup);
    if (sweep_direct) {
      bool fell_back = false;
      res = pfv::sweep_direct_solve(*h, sys, M, rtol, maxit, restart, dxs, fell_back);
      h->stats.sweep_direct_steps = 1;
      h->stats.sweep_direct_fallbacks = fell_back ? 1 : 0;
    } else {
    res = method == PFV_SOLVE_GMRES
              ? pfv::gmres_solve(*h, sys, rtol, maxit, restart, dxs, x0 == nullptr, Mp)
              : pfv::krylov_solve(*h, sys, method, rtol, maxit, dxs, x0 == nullptr, Mp);
    }
    if (M.amg && x0 == nullptr) h->amg->note_iterations(res.iterations, rtol, method, res.converged);
    h->stats.solve_launches = (int64_t)(pfv::launch_counter().load(std::memory_order_relaxed) - launches_before_loop);
    if (permuted) pfv::permute_vector(*h, (int64_t)n, h->active_bs, dxs, dx, false);
    h->stats.solve_ms = tm.stop(s);
    vec_out(h, x, dx, n);
  });
  if (info) {
    info->iterations = res.iterations;
    info->converged = res.converged ? 1 : 0;
    info->rel_residual = res.relres;
    info->solve_ms = h ? h->stats.solve_ms : 0.0;
  }
  if (st == PFV_OK && !res.converged) {
    h->err = "Krylov solver did not reach the requested tolerance";
    return PFV_ERR_NOT_CONVERGED;
  }
  return st;
}

// ---- the adjoint of the flow solve (flow_adjoint.inc).  Three parts: the checks, the maps, A^T and the right-hand side,
// ending with (A^T, g_p + T^T g_q) as the active system; pfv_solve itself; the gradients from mu.
// (grad_perm_exact: the additional output of pfv_flow_adjoint_exact, nullptr for pfv_flow_adjoint -- whose path through
// this body is the one it always took)
static pfv_status flow_adjoint_call(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                                    const double* load_flux, const double* load_pressure, int method, double rtol,
                                    int maxit, int restart, double* mu_out, double* grad_perm, double* grad_perm_exact,
                                    double* grad_bc_values, double* grad_source, pfv_solve_info* info) {
  if (info) *info = pfv_solve_info{};
  const int none = 0x7f7f7f7f;
  double *d_p = nullptr, *d_bc = nullptr, *d_gq = nullptr, *d_gp = nullptr, *d_vs = nullptr, *d_mu = nullptr;
  int32_t *first = nullptr, *last = nullptr, *ecell = nullptr;
  int vd = 0;
  double products_ms = 0.0;
  pfv_status st = guarded(h, [&] {
    require(h->have_grid && h->have_numeric && h->filled[PFV_MAT_FLUX] && h->filled[PFV_MAT_BOUND_FLUX],
            "no flow discretization on the handle: pfv_mpfa_discretize or pfv_tpfa_discretize first");
    require(p && bc_values, "p and bc_values are required");
    require(load_flux || load_pressure, "no loads: give load_flux, load_pressure or both");
    require(method == PFV_SOLVE_CG || method == PFV_SOLVE_BICGSTAB || method == PFV_SOLVE_GMRES,
            "method must be PFV_SOLVE_CG, PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    if (h->shard) throw pfv::Error(PFV_ERR_UNSUPPORTED, "the flow adjoint has no sharded form");
    if (h->periodic) throw pfv::Error(PFV_ERR_UNSUPPORTED, "the flow adjoint does not cover periodic grids");
    if (h->subface_bc)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "the flow adjoint does not cover conditions per sub-face (flux has sub-face rows)");
    if (!h->tpfa_mode && !h->rows_complete)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "the flow adjoint does not cover a partial discretization (the rows of the "
                                            "other faces are zero)");
    if (h->pat_flux.nnz >= (int64_t(1) << 31))
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "the flow adjoint needs a flux pattern below 2^31 entries");
    require(!vector_source || h->filled[PFV_MAT_VECTOR_SOURCE], "vector_source matrix was skipped");
    if (grad_perm_exact && !h->tpfa_mode) pfv::adj_check_lds(*h);  // (a region too large for the LDS: refused before the solve)
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc, ncf = (size_t)h->ncf;
    vd = (int)(h->pat_vs.ncols / h->nc);
    const size_t nvs = vector_source ? (size_t)vd * nc : 0;
    double* in = h->fa_in.ensure(2 * nc + 2 * nf + nvs);
    d_p = in;
    d_bc = in + nc;
    d_gq = load_flux ? in + nc + nf : nullptr;
    d_gp = load_pressure ? in + nc + 2 * nf : nullptr;
    d_vs = vector_source ? in + 2 * nc + 2 * nf : nullptr;
    vec_in(h, d_p, p, nc);
    vec_in(h, d_bc, bc_values, nf);
    if (d_gq) vec_in(h, d_gq, load_flux, nf);
    if (d_gp) vec_in(h, d_gp, load_pressure, nc);
    if (d_vs) vec_in(h, d_vs, vector_source, nvs);
    int32_t* half = h->fa_half.ensure(2 * nf + ncf);
    first = half;
    last = half + nf;
    ecell = half + 2 * nf;
    pfv::flow_adjoint_half_faces(*h, first, last, ecell);
    const pfv::FlowAdjointFindings fd = pfv::flow_adjoint_check(*h, first, last, d_p, d_bc, d_gq, d_gp);
    if (fd.robin != none)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "face " + std::to_string(fd.robin) + " carries a Robin condition: the flow "
                                            "adjoint covers Dirichlet and Neumann faces");
    if (fd.internal != none)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "face " + std::to_string(fd.internal) + " is flagged PFV_BC_INTERNAL: the flow "
                                            "adjoint does not cover internal boundaries");
    if (fd.bad_gq != none)
      throw pfv::Error(PFV_ERR_ARGUMENT, "load_flux[" + std::to_string(fd.bad_gq) + "] is not finite");
    if (fd.bad_gp != none)
      throw pfv::Error(PFV_ERR_ARGUMENT, "load_pressure[" + std::to_string(fd.bad_gp) + "] is not finite");
    if (fd.bad_p != none) throw pfv::Error(PFV_ERR_ARGUMENT, "p[" + std::to_string(fd.bad_p) + "] is not finite");
    if (fd.bad_bc != none)
      throw pfv::Error(PFV_ERR_ARGUMENT, "bc_values[" + std::to_string(fd.bad_bc) + "] (a boundary face) is not finite");
    // ---- what belongs to the patterns: column maps, transposed positions
    pfv::Timer tm;
    h->stats.flow_adjoint_map_ms = 0.0;
    const size_t nnzA = (size_t)std::max<int64_t>(h->pat_A.nnz, 1);
    if (!h->have_cmap || !h->have_tpos_A) {
      tm.start(s);
      if (!h->have_cmap) {
        pfv::colmap_build(*h, h->pat_flux, h->cmap_flux);
        pfv::colmap_build(*h, h->pat_bound, h->cmap_bound);
        h->have_cmap = true;
        ++h->stats.flow_adjoint_map_builds;
      }
      if (!h->have_tpos_A) {
        pfv::sweep_transpose_positions(*h, h->pat_A, h->tpos_A.ensure(nnzA), "div flux");
        h->have_tpos_A = true;
      }
      h->stats.flow_adjoint_map_ms = tm.stop(s);
    }
    // ---- A = div T afresh, A^T on its own pattern
    h->active.valid = false;  // (whatever was active: the call ends without an active system)
    if (!h->have_system) {
      h->have_advdiff = h->have_adv_bD = false;  // (as pfv_mpfa_assemble: built on the previous div @ flux)
      values_changed(h, Windows::consume);
    } else {
      values_changed(h, Windows::keep);
    }
    pfv::assemble_system(*h);
    double* valT = h->fa_valT.ensure(nnzA);
    pfv::sweep_transpose_values(*h, h->pat_A.nnz, h->tpos_A.p, h->val[PFV_MAT_SYSTEM].p, valT);
    double* rhs = h->fa_rhs.ensure(nc);
    d_mu = h->fa_mu.ensure(nc);
    tm.start(s);
    if (d_gq) {
      pfv::spmv_transposed(*h, h->cmap_flux, h->val[PFV_MAT_FLUX].p, d_gq, rhs);
      if (d_gp) {
        const double* gp = d_gp;
        pfv::parallel_for(s, (int64_t)nc, PFV_LAMBDA(int64_t i) { rhs[i] = gp[i] + rhs[i]; });
      }
    } else {
      pfv::be_d2d(rhs, d_gp, sizeof(double) * nc, s);
    }
    products_ms = tm.stop(s);
    activate(h, h->pat_A, valT, h->diag.p, rhs, h->nc, 1, true);
  });
  if (st != PFV_OK) return st;
  // ---- the solve, through the owner of the active system; mu stays on the device
  pfv_solve_info sinfo{};
  const bool on_device = h->vectors_on_device;
  h->vectors_on_device = true;
  st = pfv_solve(h, method, rtol, maxit, restart, nullptr, d_mu, &sinfo);
  h->vectors_on_device = on_device;
  h->active.valid = false;
  if (info) *info = sinfo;
  ++h->stats.flow_adjoint_calls;
  h->stats.flow_adjoint_iterations = sinfo.iterations;
  h->stats.flow_adjoint_solve_ms = sinfo.solve_ms;
  h->stats.flow_adjoint_products_ms = products_ms;
  h->stats.flow_adjoint_gradient_ms = 0.0;
  if (st != PFV_OK) return st;
  return guarded(h, [&] {
    auto s = h->stream;
    const size_t nf = (size_t)h->nf, nc = (size_t)h->nc, ncf = (size_t)h->ncf;
    pfv::Timer tm;
    h->stats.flow_adjoint_exact_map_ms = h->stats.flow_adjoint_exact_ms = 0.0;
    if (grad_perm || grad_bc_values || grad_perm_exact) {
      pfv::Buf<double> z_, zw_, inv_, gk_, gb_, ge_;
      double* z = z_.ensure(nf);
      double* zw = zw_.ensure(nf);
      // (for a TPFA discretization the two-point gradient is the exact one)
      const bool two_point = grad_perm || (grad_perm_exact && h->tpfa_mode);
      tm.start(s);
      pfv::flow_adjoint_faces(*h, first, last, ecell, d_p, d_bc, d_vs, vd, d_gq, d_mu, z, zw);
      double* gk = nullptr;
      if (two_point) {
        gk = gk_.ensure(9 * nc);
        pfv::flow_adjoint_grad_perm(*h, first, last, zw, inv_.ensure(std::max<size_t>(ncf, 1)), gk);
      }
      h->stats.flow_adjoint_gradient_ms = tm.stop(s);
      double* ge = nullptr;
      if (grad_perm_exact && !h->tpfa_mode) {
        tm.start(s);
        if (adj_ensure_cell_map(h)) h->stats.flow_adjoint_exact_map_ms = tm.stop(s);
        ge = ge_.ensure(9 * nc);
        tm.start(s);
        pfv::flow_adjoint_grad_perm_exact(*h, d_p, d_bc, d_vs, vd, z, ge);
        h->stats.flow_adjoint_exact_ms = tm.stop(s);
        ++h->stats.flow_adjoint_exact_calls;
      }
      if (grad_perm) vec_out(h, grad_perm, gk, 9 * nc);
      if (grad_perm_exact) vec_out(h, grad_perm_exact, ge ? ge : gk, 9 * nc);
      if (grad_bc_values) {
        double* gb = gb_.ensure(nf);
        tm.start(s);
        pfv::spmv_transposed(*h, h->cmap_bound, h->val[PFV_MAT_BOUND_FLUX].p, z, gb);
        h->stats.flow_adjoint_products_ms += tm.stop(s);
        vec_out(h, grad_bc_values, gb, nf);
      }
      pfv::be_sync(s);  // (the staging buffers are freed on return)
    }
    if (mu_out) vec_out(h, mu_out, d_mu, nc);
    if (grad_source) vec_out(h, grad_source, d_mu, nc);
    pfv::be_sync(s);
  });
}

pfv_status pfv_flow_adjoint(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                            const double* load_flux, const double* load_pressure, int method, double rtol, int maxit,
                            int restart, double* mu_out, double* grad_perm, double* grad_bc_values,
                            double* grad_source, pfv_solve_info* info) {
  return flow_adjoint_call(h, p, bc_values, vector_source, load_flux, load_pressure, method, rtol, maxit, restart, mu_out,
                           grad_perm, nullptr, grad_bc_values, grad_source, info);
}

pfv_status pfv_flow_adjoint_exact(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                                  const double* load_flux, const double* load_pressure, int method, double rtol,
                                  int maxit, int restart, double* mu_out, double* grad_perm, double* grad_perm_exact,
                                  double* grad_bc_values, double* grad_source, pfv_solve_info* info) {
  return flow_adjoint_call(h, p, bc_values, vector_source, load_flux, load_pressure, method, rtol, maxit, restart, mu_out,
                           grad_perm, grad_perm_exact, grad_bc_values, grad_source, info);
}


pfv_status pfv_solve_sharded(pfv_ctx* h, int method, double rtol, int maxit, int64_t n_own,
                             const pfv_shard_hooks* hooks, double* d_work, double* d_x_owned,
                             pfv_solve_info* info) {
  pfv::SolveResult res;
  pfv_status st = guarded(h, [&] {
    if (h->precond == PFV_PRECOND_AMG_NNS)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_AMG_NNS has no sharded form: pfv_set_preconditioner(PFV_PRECOND_AMG) "
                                            "or PFV_PRECOND_JACOBI for sharded solves");
    if (h->precond == PFV_PRECOND_SWEEP)
      throw pfv::Error(PFV_ERR_UNSUPPORTED, "PFV_PRECOND_SWEEP has no AMG hierarchy and no sharded form");
    require(h->active.valid, "assemble first");
    require(hooks && hooks->exchange_halo && hooks->allreduce_sum, "both hooks are required");
    require(d_work && d_x_owned, "work space and x are required");
    require(method == PFV_SOLVE_CG || method == PFV_SOLVE_BICGSTAB, "a sharded solve runs PFV_SOLVE_CG or PFV_SOLVE_BICGSTAB");
    require(rtol > 0 && maxit > 0, "rtol and maxit must be positive");
    const int64_t n_loc = h->active.n;
    require(n_own > 0 && n_own <= n_loc && n_own % h->active_bs == 0, "n_own out of range");
    auto s = h->stream;
    pfv::Timer tm;
    tm.start(s);
    const pfv::CsrPattern& P = *h->active.P;
    RowsView rows(P, n_own);
    pfv::LinSys sys = h->active;
    sys.P = &rows.V;
    sys.n = n_own;
    sys.win = nullptr;
    if (P.nnz >= pfv::env_int("PFV_SPMV_WINDOW_MIN_NNZ", 20000)) {
      if (h->win_rows_for != P.indices.p || h->win_rows_n != n_own) {
        h->win_rows_checksum = 0;
        pfv::win_build(*h, rows.V, h->win_rows);
        h->win_rows_for = P.indices.p;
        if (h->win_rows.ok && &P == &h->pat_A && h->have_symbolic) h->win_rows_checksum = h->pat_A_checksum;
        h->win_rows_n = n_own;
      }
      if (h->win_rows.ok) sys.win = &h->win_rows;
    }
    pfv::Precond M;
    const pfv::Precond* Mp = nullptr;
    if (h->precond == PFV_PRECOND_AMG) {
      require(h->amg_block && h->amg_block->valid && h->amg_block->lev[0]->n == n_own,
              "pfv_amg_setup(n_own) first: the sharded solve preconditions with the hierarchy of the owned block");
      M.amg = h->amg_block.get();
      Mp = &M;
    } else if (h->precond == PFV_PRECOND_BLOCK) {
      // block lower-triangular sweep over the blocks of the OWNED unknowns (pfv_set_block_preconditioner with a layout
      // that covers [0, n_own)): couplings to other ranks' unknowns are left to the Krylov loop (block Jacobi across
      // ranks, Gauss-Seidel over the (variable, subdomain) blocks inside a rank) -- every diagonal block is extracted
      // from the owned rows and columns, the halo columns lie behind them and never enter a block or its sweep
      require(h->block_pc != nullptr, "pfv_set_block_preconditioner first");
      require(h->block_pc->ptr.back() == n_own, "the block layout must cover exactly the owned unknowns");
      if (h->block_pc->for_val != sys.val) {
        pfv::blockpc_setup(*h, *h->block_pc, rows.V, sys.val);
        h->stats.amg_setup_ms = h->block_pc->setup_ms;
      }
      M.blocks = h->block_pc.get();
      M.P = &rows.V;
      M.val = sys.val;
      M.diag = sys.diag;
      Mp = &M;
    }
    pfv::be_memset(d_x_owned, 0, sizeof(double) * (size_t)n_own, s);
    pfv::be_memset(d_work, 0, sizeof(double) * (size_t)(2 * n_loc + 8), s);
    h->shard_overlap = false;
#ifndef PFV_EMULATE
    {
      // PFV_SHARD_OVERLAP=1: halo exchange of the Krylov products on the second stream beside the row blocks that need
      // no halo entry (linalg.inc: shard_spmv) -- with the native RCCL hooks only (a caller's hooks are not known to
      // honour a foreign stream).  OFF by default: no two-GPU box has run it yet.  =2 (tests): every second block
      // counts as a boundary block.
      const int ov = pfv::env_int("PFV_SHARD_OVERLAP", 0);
      if (ov != 0 && sys.win && sys.win->ok && h->aux_stream && hooks->exchange_halo == &pfv::rccl_exchange_halo) {
        const pfv::WinCsr& W = *sys.win;
        const int64_t nblk = W.nblk;
        int32_t* lst = h->shard_blocks.ensure(2 * nblk + 2);
        int32_t* cnt = h->status.ensure(16);
        pfv::be_memset(cnt + 12, 0, 2 * sizeof(int32_t), s);
        const int64_t* wptr = W.wptr64;
        const int32_t* wlen = W.wlen;
        const int32_t* wcol = W.wcol.p;
        int32_t* tmp_b = lst + nblk;  // boundary blocks collected behind, moved up below
        pfv::parallel_for(s, nblk, PFV_LAMBDA(int64_t b) {
          const int64_t w0 = wptr[b];
          const int wn = wlen ? wlen[b] : (int)(wptr[b + 1] - w0);
          const bool bnd = ov == 2 ? (b & 1) != 0 : (wn > 0 && wcol[w0 + wn - 1] >= n_own);  // (window columns ascend)
          if (bnd) tmp_b[atomicAdd(cnt + 13, 1)] = (int32_t)b;
          else lst[atomicAdd(cnt + 12, 1)] = (int32_t)b;
        });
        int32_t hc[2];
        be_d2h(hc, cnt + 12, sizeof(hc), s);
        h->shard_n_interior = hc[0];
        h->shard_n_boundary = hc[1];
        pfv::be_d2d(lst + hc[0], tmp_b, sizeof(int32_t) * (size_t)hc[1], s);
        h->shard_overlap = true;
      }
    }
#endif
    h->shard = hooks;
    h->shard_work = d_work;
    h->shard_nloc = n_loc;
    try {
      res = pfv::krylov_solve(*h, sys, method, rtol, maxit, d_x_owned, true, Mp);
    } catch (...) {
      h->shard = nullptr;
      throw;
    }
    h->shard = nullptr;
    if (M.amg) h->amg_block->note_iterations(res.iterations, rtol, method, res.converged);
    h->stats.solve_ms = tm.stop(s);
  });
  if (info) {
    info->iterations = res.iterations;
    info->converged = res.converged ? 1 : 0;
    info->rel_residual = res.relres;
    info->solve_ms = h ? h->stats.solve_ms : 0.0;
  }
  if (st == PFV_OK && !res.converged) {
    h->err = "Krylov solver did not reach the requested tolerance";
    return PFV_ERR_NOT_CONVERGED;
  }
  return st;
}

pfv_status pfv_sweep_info(pfv_ctx* h, int64_t info[4], int32_t* level, int32_t* order) {
  return guarded(h, [&] {
    require(h->sweep && h->sweep->valid, "no flow order on the handle (a solve with PFV_PRECOND_SWEEP builds it)");
    const pfv::Sweep& sw = *h->sweep;
    if (info) {
      info[0] = sw.nc;
      info[1] = sw.nlev;
      info[2] = sw.n_core;
      info[3] = sw.core_level;
    }
    if (level) be_d2h(level, sw.level.p, sizeof(int32_t) * (size_t)sw.nc, h->stream);
    if (order) be_d2h(order, sw.order.p, sizeof(int32_t) * (size_t)sw.nc, h->stream);
  });
}

pfv_status pfv_get_stats(pfv_ctx* h, pfv_stats* out) {
  return guarded(h, [&] {
    require(out != nullptr, "null output");
    *out = h->stats;
  });
}

pfv_status pfv_get_stats_n(pfv_ctx* h, void* out, size_t struct_size) {
  return guarded(h, [&] {
    require(out != nullptr, "null output");
    std::memcpy(out, &h->stats, std::min(struct_size, sizeof(pfv_stats)));
  });
}

pfv_status pfv_time_kernel(pfv_ctx* h, int kernel, int reps, double* avg_ms) {
  return guarded(h, [&] {
    require(avg_ms != nullptr && reps > 0, "bad argument");
    auto s = h->stream;
    pfv::Timer tm;
    if (kernel == PFV_KERNEL_SPMV_A) {
      require(h->have_system && h->have_flow_rhs, "assemble first");
      const size_t n = (size_t)h->nc;
      double* x = h->kry[7].ensure(n);
      double* y = h->kry[8].ensure(n);
      pfv::be_d2d(x, h->rhs.p, n * sizeof(double), s);
      // what the Krylov loop launches (renumbered system, windowed kernel when the pattern allows it)
      require(active_is(h, PFV_MAT_SYSTEM) && h->active.P == &h->pat_A, "the flow system must be the active one");
      bool permuted = false;
      const pfv::LinSys sys = solver_system(h, permuted);
      pfv::sys_spmv(*h, sys, x, y);
      tm.start(s);
      for (int i = 0; i < reps; ++i) pfv::sys_spmv(*h, sys, x, y);
      *avg_ms = tm.stop(s) / reps;
    } else if (kernel == PFV_KERNEL_AMG_SMOOTH) {
      pfv::Amg* amg = (h->amg && h->amg->valid) ? h->amg.get() : h->amg_block.get();  // single-GPU / sharded
      require(amg && amg->valid && amg->nlev > 0, "no AMG hierarchy (solve with PFV_PRECOND_AMG first)");
      pfv::AmgLevel& L = *amg->lev[0];
      const size_t n = (size_t)std::max(L.n, L.m);  // (coupled hierarchy: the input carries the halo entries)
      double* x = h->kry[7].ensure(n);
      double* y = h->kry[8].ensure(n);
      double* b = h->kry[6].ensure(n);
      pfv::be_memset(x, 0, n * sizeof(double), s);
      pfv::be_memset(b, 0, n * sizeof(double), s);
      pfv::amg_spmv(*h, *amg, L, x, y, b);
      tm.start(s);
      for (int i = 0; i < reps; ++i) pfv::amg_spmv(*h, *amg, L, x, y, b);
      *avg_ms = tm.stop(s) / reps;
    } else if (kernel == PFV_KERNEL_TRIAD) {
      const size_t n = size_t(1) << 27;
      pfv::Buf<double> buf;
      double* a = buf.ensure(3 * n);
      double* b = a + n;
      double* cc = b + n;
      pfv::be_memset(a, 0, 3 * n * sizeof(double), s);
      pfv::D2* a2 = reinterpret_cast<pfv::D2*>(a);
      const pfv::D2* b2 = reinterpret_cast<const pfv::D2*>(b);
      const pfv::D2* c2 = reinterpret_cast<const pfv::D2*>(cc);
      auto triad = [&] {  // 16 bytes per lane and stream, four independent loads per stream in flight
#ifdef PFV_EMULATE
        for (size_t i = 0; i < n / 2; ++i) {
          a2[i].x = b2[i].x + 0.5 * c2[i].x;
          a2[i].y = b2[i].y + 0.5 * c2[i].y;
        }
#else
        PFV_LAUNCH(pfv::k_triad, dim3(256 * 16), dim3(256), 0, s, (int64_t)(n / 2), a2, b2, c2);
        PFV_HIP_CHECK(hipGetLastError());
#endif
      };
      triad();
      tm.start(s);
      for (int i = 0; i < reps; ++i) triad();
      *avg_ms = tm.stop(s) / reps;
    } else if (kernel == PFV_KERNEL_READ) {
#ifdef PFV_EMULATE
      *avg_ms = 0.0;
#else
      const size_t n = size_t(1) << 28;
      pfv::Buf<double> buf;
      double* a = buf.ensure(n + 8);
      pfv::be_memset(a, 0, (n + 8) * sizeof(double), s);
      auto rd = [&] {
        PFV_LAUNCH(pfv::k_read_stream, dim3(256 * 16), dim3(256), 0, s, (int64_t)(n / 2),
                           reinterpret_cast<const pfv::D2*>(a), a + n);
        PFV_HIP_CHECK(hipGetLastError());
      };
      rd();
      tm.start(s);
      for (int i = 0; i < reps; ++i) rd();
      *avg_ms = tm.stop(s) / reps;
#endif
    } else if (kernel == PFV_KERNEL_NODE) {
      require(h->have_numeric, "discretize first");
      tm.start(s);
      for (int i = 0; i < reps; ++i) pfv::run_node_kernel(*h);
      *avg_ms = tm.stop(s) / reps;
    } else if (kernel == PFV_KERNEL_FACE) {
      require(h->have_numeric, "discretize first");
      const bool with_vs = h->filled[PFV_MAT_VECTOR_SOURCE];
      tm.start(s);
      for (int i = 0; i < reps; ++i) pfv::run_face_kernel(*h, with_vs);
      *avg_ms = tm.stop(s) / reps;
    } else {
      require(false, "unknown kernel id");
    }
  });
}

pfv_status pfv_debug_copy(pfv_ctx* h, int which, double* dst, int64_t count) {
  return guarded(h, [&] {
    require(h->have_numeric && dst && count >= 0 && count <= (which == 0 ? h->tab_len : h->tabb_len), "bad argument");
    const double* src = which == 0 ? h->tab.p : h->tabb.p;
    be_d2h(dst, src, sizeof(double) * (size_t)count, h->stream);
  });
}

pfv_status pfv_debug_topology(pfv_ctx* h, int which, void* dst, int64_t capacity, int64_t* bytes) {
  return guarded(h, [&] {
    require(h->have_topology && bytes && which >= 0 && which <= 20, "bad argument");
    auto s = h->stream;
    const int64_t nn = h->nn, nf = h->nf, nsf = h->nsf, nh = h->nh;
    const void* src = nullptr;
    int64_t n = 0;
    std::vector<int64_t> host;
    switch (which) {
      case 0: src = h->node_hptr.p; n = 4 * (nn + 1); break;
      case 1: src = h->h_cell.p; n = 4 * nh; break;
      case 2: src = h->h_lf.p; n = nh; break;
      case 3: src = h->h_sgn.p; n = nh; break;
      case 4: src = h->h_first.p; n = nh; break;
      case 5: src = h->node_fptr.p; n = 4 * (nn + 1); break;
      case 6: src = h->node_sf.p; n = 4 * nsf; break;
      case 7: src = h->sf_face.p; n = 4 * nsf; break;
      case 8: src = h->sf_ls.p; n = nsf; break;
      case 9: src = h->face_nsides.p; n = 4 * nf; break;
      case 10: src = h->node_face.p; n = 4 * nsf; break;
      case 11: src = h->node_bptr.p; n = 4 * (nn + 1); break;
      case 12:
      case 13: {
        const int64_t nb = pfv::read_scalar<int32_t>(s, h->node_bptr.p + nn);
        src = which == 12 ? (const void*)h->node_bfaces.p : (const void*)h->node_bls.p;
        n = which == 12 ? 4 * nb : nb;
        break;
      }
      case 14: src = h->node_tptr.p; n = 8 * (nn + 1); break;
      case 15: src = h->node_tbptr.p; n = 8 * (nn + 1); break;
      case 16: src = h->node_cells.p; n = 4 * (nh / h->nd); break;
      case 17: src = h->face_order.p; n = 4 * nf; break;
      case 18: src = h->node_order.p; n = 4 * nn; break;
      case 19: host.assign(h->class_begin.begin(), h->class_begin.end()); break;
      default: {
        int64_t flops_bits = 0;
        std::memcpy(&flops_bits, &h->stats.node_flops, sizeof(double));
        host = {nh, h->max_face_nodes, h->max_cell_faces, h->max_block, h->max_deg, h->max_bnd_per_node,
                h->sum_block_sq, h->tab_len, h->tabb_len, flops_bits, (int64_t)h->stats.num_nodes,
                (int64_t)h->stats.num_sub_half_faces, (int64_t)h->stats.sum_block_sq, (int64_t)h->stats.max_block,
                (int64_t)h->stats.node_table_doubles, (int64_t)pfv::topology_digest(*h), (int64_t)h->topo_path};
        break;
      }
    }
    if (which >= 19) n = 8 * (int64_t)host.size();
    *bytes = n;
    if (dst && capacity >= n && n > 0) {
      if (which >= 19) std::memcpy(dst, host.data(), (size_t)n);
      else be_d2h(dst, src, (size_t)n, s);
    }
  });
}

}  // extern "C"

#include "rccl_hooks.inc"
#include "csr_algebra.inc"
