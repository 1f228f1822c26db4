/* porefv.h — C ABI of libporefv_hip.so: MI355X-native MPFA-O assembly + sparse solve.
 *
 * This is the drop-in boundary for PorePy's finite-volume hot path.  PorePy is pure
 * Python, so the binding a maintainer adds is a ctypes stub; each
 * entry point names the reference code it stands in for (paths relative to
 * /root/reference/src/porepy).  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - every function returns a pfv_status (0 = ok); pfv_last_error() gives the text
 *   - all floating point is FP64, all indices int32 (CSR outputs as scipy stores them)
 *   - geometry arrays are SoA with 3 rows, row-major: a[3][N]   (Grid.nodes etc.)
 *   - "host" pointers are read/written synchronously; the handle owns all device memory
 *   - one handle = one HIP device + one stream; calls on a handle are blocking and
 *     must not be issued concurrently (the reference is single-threaded too)
 */
#ifndef POREFV_H
#define POREFV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfv_ctx pfv_ctx;

typedef enum {
  PFV_OK = 0,
  PFV_ERR_SINGULAR = 1,      /* ValueError("Error in inversion of local linear systems"),
                                numerics/linalg/matrix_operations.py:1487-1490 */
  PFV_ERR_CELL_SHAPE = 2,    /* AssertionError: != nd faces of a cell meet in a node,
                                numerics/fv/_fvutils.py:735-736 */
  PFV_ERR_HIP = 3,           /* HIP runtime error; text in pfv_last_error */
  PFV_ERR_ARGUMENT = 4,      /* bad argument / call order */
  PFV_ERR_UNSUPPORTED = 5,   /* size or feature outside what the kernels cover */
  PFV_ERR_NOT_CONVERGED = 6  /* Krylov solve hit maxit (solution still returned) */
} pfv_status;

/* matrix selectors; 0..5 are the six keys FVElliptic stores
 * (numerics/fv/fv_elliptic.py:30-53), 6 is A = div @ flux (fv_elliptic.py:90-96) */
enum {
  PFV_MAT_FLUX = 0,
  PFV_MAT_BOUND_FLUX = 1,
  PFV_MAT_BOUND_PRESSURE_CELL = 2,
  PFV_MAT_BOUND_PRESSURE_FACE = 3,
  PFV_MAT_VECTOR_SOURCE = 4,
  PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE = 5,
  PFV_MAT_SYSTEM = 6,
  /* MPSA: the four keys Mpsa stores (numerics/fv/mpsa.py:82-95) and A = div_nd @ stress
   * (mpsa.py:515-529); vector unknowns are cell-major, component-minor (u[nd*c + a]) */
  PFV_MAT_STRESS = 7,
  PFV_MAT_BOUND_STRESS = 8,
  PFV_MAT_BOUND_DISPLACEMENT_CELL = 9,
  PFV_MAT_BOUND_DISPLACEMENT_FACE = 10,
  PFV_MAT_MECH_SYSTEM = 11,
  PFV_MAT_USER_SYSTEM = 12, /* matrix handed over by pfv_set_system */
  PFV_MAT_FLUX_JACOBIAN = 13, /* d flux / d p of pfv_mpfa_ad_flux_system, on the pattern of flux */
  /* Upwind.discretize (numerics/fv/upwind.py:165-335): "transport" (k Nf x k Nc), "rhs_dir", "rhs_neu" (k Nf x k Nf),
   * and the advective system A = div diag(q) U of Upwind.assemble_matrix_rhs (upwind.py:67-163) */
  PFV_MAT_UPWIND = 14,
  PFV_MAT_UPWIND_RHS_DIR = 15,
  PFV_MAT_UPWIND_RHS_NEU = 16,
  PFV_MAT_TRANSPORT_SYSTEM = 17,
  PFV_MAT_ADVDIFF_SYSTEM = 18, /* diag(acc) + div flux + w div diag(q) U of pfv_advdiff_assemble, on the pattern of
                                  PFV_MAT_SYSTEM */
  PFV_NUM_MATS = 19
};

/* boundary-condition flag bits per face (params/bc.py:68-190: is_dir/is_neu/is_rob/
 * is_internal of BoundaryCondition) */
enum { PFV_BC_DIR = 1, PFV_BC_NEU = 2, PFV_BC_ROB = 4, PFV_BC_INTERNAL = 8 };

/* Krylov methods for pfv_solve (the reference only has direct solvers,
 * models/solution_strategy.py:830-884; results are judged against its solution) */
enum { PFV_SOLVE_CG = 0, PFV_SOLVE_BICGSTAB = 1, PFV_SOLVE_GMRES = 2 };

/* preconditioners of pfv_solve: Jacobi (default), or one V(1,1) cycle of a plain-aggregation
 * algebraic multigrid built on the device from the assembled matrix (pairwise matching on the
 * strength graph, piecewise-constant prolongation, Galerkin coarse matrices) */
enum { PFV_PRECOND_JACOBI = 0, PFV_PRECOND_AMG = 1, PFV_PRECOND_BLOCK = 2,
       PFV_PRECOND_AMG_NNS = 3, /* aggregation AMG whose tentative prolongator carries a near-null space
                                   (pfv_set_near_null_space; rigid-body modes for elasticity) */
       PFV_PRECOND_SWEEP = 4    /* one substitution in flow order (csrc/sweep.inc): transport and advection-diffusion
                                   systems only; exact for the transport system of an acyclic flux (see pfv_sweep_info) */ };

/* flux functions f(s) of pfv_transport_advance_nl (csrc/fluxfn.h), nondecreasing on [0, 1] */
enum {
  PFV_FLUXFN_LINEAR = 0, /* f(s) = s, no parameters: the linear transport step */
  PFV_FLUXFN_COREY = 1,  /* 6 parameters s_wr, s_nr, n_w, n_n, mu_w, mu_n: s_e = clamp((s - s_wr) / (1 - s_wr - s_nr), 0, 1),
                            f = l_w / (l_w + l_n) with l_w = s_e^n_w / mu_w, l_n = (1 - s_e)^n_n / mu_n */
  PFV_FLUXFN_TABLE = 2   /* m = 2 .. 1024 finite, nondecreasing values on uniform knots over [0, 1], piecewise linear */
};

/* sorption isotherms S(c), c >= 0, of pfv_transport_advance_sorb (csrc/isotherm.h): two parameters each, S(0) = 0,
 * nondecreasing */
enum {
  PFV_ISOTHERM_LINEAR = 0,     /* S = Kd c: Kd >= 0, the second parameter is not read */
  PFV_ISOTHERM_FREUNDLICH = 1, /* S = Kf c^n: Kf >= 0, n > 0 (n < 1: an infinite slope at c = 0, taken from c = 0 on) */
  PFV_ISOTHERM_LANGMUIR = 2    /* S = q_max b c / (1 + b c): q_max >= 0, b >= 0 */
};

/* flags for pfv_mpfa_discretize */
enum {
  PFV_DISCR_REBUILD_TOPOLOGY = 1, /* redo sub-cell topology + CSR symbolic phase even if
                                     cached (what every Mpfa.discretize call does) */
  PFV_DISCR_SKIP_VECTOR_SOURCE = 2 /* do not fill matrices 4 and 5 */
};

typedef struct {
  int32_t iterations;
  int32_t converged;
  double rel_residual; /* ||b - A x|| / ||b|| as tracked by the recurrence */
  double solve_ms;     /* device time of the solve (HIP events) */
} pfv_solve_info;

/* phase timings of the last calls, milliseconds, measured with HIP events on the
 * handle's stream (the reference logs wall-clock per phase:
 * models/solution_strategy.py:435-442,807-828,846-884) */
typedef struct {
  double topology_ms;     /* SubcellTopology equivalent          (_fvutils.py:51-172)   */
  double symbolic_ms;     /* CSR patterns of the 6 matrices + A                            */
  double node_ms;         /* interaction-region kernel            (mpfa.py:997-1045)     */
  double face_ms;         /* stencil scatter into CSR             (mpfa.py:1088-1147)    */
  double assemble_ms;     /* div @ flux, rhs                      (fv_elliptic.py:67-112) */
  double solve_ms;
  double bytes_written_outputs; /* 8*nnz (+4*nnz per distinct pattern) of what was filled */
  int64_t num_nodes, num_sub_half_faces, sum_block_sq, max_block;
  double amg_setup_ms;            /* last AMG hierarchy build */
  double amg_operator_complexity; /* sum of nnz over the levels / nnz of the system */
  int64_t amg_levels, amg_coarsest_rows;
  double discretize_ms;           /* whole pfv_mpfa_discretize call; less than the sum of its phases when the
                                     interaction-region kernel ran beside the symbolic phase on the handle's
                                     second stream (symbolic_ms and node_ms then are overlapping spans) */
  int64_t solve_renumbered;       /* 1: the last pfv_solve worked on the copy renumbered along the Morton curve,
                                     0: in place (grid already numbered that way, or a user system) */
  double node_flops;              /* FP64 operations the interaction-region kernel executes per launch on this grid:
                                     sum over the nodes of 2 n^3 (Gauss-Jordan) + 2 nd n nh (response table)
                                     + 2 nd nh (3 n_b) (boundary columns) + ~60 nd^2 per sub-cell (nK, D^-1, omega) */
  int64_t node_table_doubles;     /* doubles in the per-node response tables (what the node kernel writes and the
                                     face kernel reads) */
  int64_t amg_maps_reused;        /* 1: the last AMG setup kept the aggregates of the previous one (same pattern,
                                     new values: only the Galerkin products were redone), 0: full setup */
  int64_t amg_level0_nnz;         /* entries of the matrix the finest level of the cycle smooths with: nnz of the system,
                                     or of its strength-filtered copy (PFV_AMG_FILTER_PERMIL, scalar systems: default) */
  double amg_filter_theta;        /* threshold of that filter (0: off) */
  int64_t win_reused;             /* 1: the last discretize kept the SpMV windows of A -- the symbolic phase proved A's
                                     pattern equal (sizes + checksum of the index arrays) to the one they were built for */
  int64_t amg_filter_layout;      /* last AMG setup's strength filter: 0 counted and scanned the kept entries, 1 wrote into
                                     the row layout of the previous filtering of the same pattern (every row kept as many
                                     entries as its slot held), 2 tried that, found a row that did not, and ran again */
  int64_t solve_launches;         /* kernel dispatches of the last pfv_solve's Krylov loop, preconditioner applications
                                     included, its setup excluded (this library's own kernels; rocPRIM primitives, memsets
                                     and copies are not counted) */
  int64_t amg_setup_launches;     /* ... of the last preconditioner setup */
  int64_t node_redo;              /* interaction regions the first launch of the last discretization handed to the
                                     pivoted full body: those whose unpivoted elimination failed its a-posteriori check
                                     (PFV_NODE_GJ=5) */
  int64_t symbolic_reused;        /* 1: the last discretize with PFV_DISCR_REBUILD_TOPOLOGY rebuilt the topology, proved it
                                     equal (64-bit digest of what the symbolic phase reads + sizes) to the one the CSR
                                     patterns on the handle were built from, and kept them; symbolic_ms then is the time of
                                     the proof.  0: the patterns were rebuilt (first call, new grid, PFV_SYMB_REUSE=0) */
  int64_t amg_stale_rematches;    /* times a solve on KEPT aggregate maps needed more than 1.3 x the iterations of the first
                                     solve after their matching (same tolerance and method): the maps were dropped and the
                                     next setup matched again */
  int64_t mpsa_contrast_regions;  /* MPSA: interaction regions of the last discretization whose sub-cells' stiffness scales
                                     differ by more than PFV_MPSA_CONTRAST_LIMIT (1e6) -- the regions that were assembled and
                                     eliminated in double-double arithmetic (mpsa_dd.inc) */
  double mpsa_max_contrast;       /* MPSA: the largest such ratio over all interaction regions (1: homogeneous) */
  int64_t assemble_positions_kept; /* 1: the last div @ flux replayed the positions of its entries recorded under the same
                                      kept patterns (no column indices read, no searches); 0: searched */
  int64_t pipeline_runs;          /* always 0 (kept so that the fields after it keep their offsets) */
  int64_t amg_nns_modes;          /* modes per aggregate of the last PFV_PRECOND_AMG_NNS setup (0: none); that setup also
                                     fills amg_setup_ms, amg_operator_complexity, amg_levels and amg_coarsest_rows */
  double face_flux_ms;            /* last pfv_mpfa_face_flux (kernel only, HIP events) */
  double upwind_ms;               /* last pfv_upwind_discretize */
  double transport_assemble_ms;   /* last pfv_upwind_assemble */
  double transport_advance_ms;    /* last pfv_transport_advance, all steps */
  int64_t transport_iterations;   /* ... Krylov iterations summed over its steps */
  int64_t transport_gmres_retries; /* ... steps whose BiCGStab solve broke down (NaN residual) and were solved again with
                                      GMRES from the kept state */
  double advdiff_assemble_ms;     /* last pfv_advdiff_assemble: the refresh (and, on the first call after a discretization,
                                     the diffusion part of the right-hand side and the pattern check) */
  double advdiff_advance_ms;      /* last pfv_advdiff_advance, all steps */
  int64_t advdiff_iterations;     /* ... Krylov iterations summed over its steps */
  int64_t advdiff_precond_fallbacks; /* ... steps whose AMG-preconditioned solve did not converge and were solved again
                                        with Jacobi-GMRES from the kept state */
  int64_t advdiff_gmres_retries;  /* ... steps whose BiCGStab solve broke down (NaN residual) and were solved again with
                                     GMRES from the kept state (pfv_transport_advance keeps its own count) */
  int64_t sweep_levels;           /* PFV_PRECOND_SWEEP, last pfv_solve: levels of the flow order (0: another preconditioner) */
  int64_t sweep_core_cells;       /* ... cells of its cyclic core (0: the flux graph is acyclic) */
  int64_t sweep_launches;         /* ... kernel dispatches of one application of the sweep */
  double sweep_order_ms;          /* ... time that solve spent building the flow order (0: it was there already); after
                                     pfv_transport_advance / pfv_advdiff_advance: summed over the steps */
  int64_t sweep_direct_steps;     /* ... 1 when that solve was the direct one (one sweep + one true-residual check, no Krylov
                                     loop); after pfv_transport_advance: the number of such steps */
  int64_t sweep_direct_fallbacks; /* ... direct solves whose residual check failed and that went on with sweep-preconditioned
                                     GMRES from the swept x (counted the same way) */
  int64_t transport_multi_components; /* last pfv_transport_advance_multi: n_comp */
  int64_t transport_multi_direct_steps; /* ... steps taken entirely by one sweep and one residual check of all components */
  int64_t transport_multi_fallback_components; /* ... component-steps solved by that component's own pfv_upwind_assemble +
                                                  pfv_transport_advance (another preconditioner, a cyclic core, a failed check) */
  double transport_nl_ms;         /* last pfv_transport_advance_nl or pfv_transport_advance_nl_multi, all steps (HIP events) */
  int64_t transport_nl_steps;     /* ... accepted steps */
  int64_t transport_nl_core_iterations; /* ... nonlinear Jacobi iterations of the cyclic core, summed over the steps */
  int64_t transport_nl_components; /* ... k of pfv_transport_advance_nl_multi, 0 after pfv_transport_advance_nl */
  double transport_react_ms;      /* last pfv_transport_advance_react, all steps (HIP events) */
  int64_t transport_react_steps;  /* ... accepted steps */
  int64_t transport_react_core_iterations; /* ... block Jacobi iterations of the cyclic core, summed over the steps */
  int64_t transport_react_components; /* ... its k */
  double transport_adjoint_ms;    /* last pfv_transport_adjoint_multi, all steps (HIP events) */
  int64_t transport_adjoint_steps; /* ... accepted adjoint steps */
  int64_t transport_adjoint_core_iterations; /* ... Jacobi iterations of the cyclic core, summed over the steps */
  int64_t amg_ap_nnz;             /* entries of AP = A_s P of the last AMG setup: the matrix the post-smoothing step of the
                                     cycle's finest level reads in place of a second sweep over the level's operator
                                     (PFV_AMG_POST_AP, default on; its build is part of amg_setup_ms).  0: that level takes the
                                     prolongation and the smoothing product as two launches (block systems, sharded solves,
                                     PFV_AMG_FP32=0, a finest level small enough for the fused restriction) */
  double transport_react_adjoint_ms; /* last pfv_transport_adjoint_react, all steps (HIP events) */
  int64_t transport_react_adjoint_steps; /* ... accepted adjoint steps */
  int64_t transport_react_adjoint_core_iterations; /* ... block Jacobi iterations of the cyclic core, summed over the steps */
  int64_t amg_galerkin_ap;        /* 1: the last AMG setup formed the first coarse operator as P^T (A_s P), one Galerkin product
                                     over AP (PFV_AMG_GALERKIN_AP, default on: scalar systems on kept aggregate maps whose AP is
                                     built).  0: the pairwise passes formed it (first setup, changed pattern or matching
                                     switches, block systems, sharded solves, PFV_AMG_FP32=0, PFV_AMG_POST_AP=0) */
  double transport_nl_adjoint_ms; /* last pfv_transport_adjoint_nl, all steps (HIP events) */
  int64_t transport_nl_adjoint_steps; /* ... accepted adjoint steps */
  int64_t transport_nl_adjoint_core_iterations; /* ... Jacobi iterations of the cyclic core, summed over the steps */
  double transport_nlc_adjoint_ms; /* last pfv_transport_adjoint_nl_multi, all steps (HIP events) */
  int64_t transport_nlc_adjoint_steps; /* ... accepted adjoint steps */
  int64_t transport_nlc_adjoint_core_iterations; /* ... Jacobi iterations of the cyclic core, summed over the steps */
  int64_t flow_adjoint_calls;      /* pfv_flow_adjoint calls on this handle that reached their solve */
  int64_t flow_adjoint_iterations; /* Krylov iterations of the last one */
  int64_t flow_adjoint_map_builds; /* times the column maps of flux / bound_flux were built (kept with the patterns) */
  double flow_adjoint_map_ms;      /* last pfv_flow_adjoint: column maps and transposed positions (0: kept) */
  double flow_adjoint_products_ms; /* ... the two transposed products T^T g_q and B^T z */
  double flow_adjoint_solve_ms;    /* ... the transposed solve, preconditioner set-up included */
  double flow_adjoint_gradient_ms; /* ... the face kernel and the cell kernel of grad_perm */
  double advdiff_adjoint_ms;       /* last pfv_advdiff_adjoint: everything after its checks, up to the copies out */
  int64_t advdiff_adjoint_steps;   /* ... adjoint steps accepted */
  int64_t advdiff_adjoint_iterations; /* ... Krylov iterations summed over its steps */
  int64_t advdiff_adjoint_gmres_retries; /* ... steps whose BiCGStab solve broke down (NaN residual) and were solved
                                     again with GMRES */
  int64_t advdiff_adjoint_precond_fallbacks; /* ... steps whose AMG-preconditioned solve did not converge and were
                                     solved again with Jacobi-GMRES */
  double advdiff_adjoint_accumulate_ms; /* ... HIP-event time of the face pass and the cell pass, summed over the steps */
  int64_t flow_adjoint_exact_calls; /* pfv_flow_adjoint_exact calls on this handle that ran the interaction-region pass */
  int64_t flow_adjoint_exact_map_builds; /* times the cell -> sub-cell map was built (kept with the sub-cell topology) */
  double flow_adjoint_exact_map_ms; /* last pfv_flow_adjoint / pfv_flow_adjoint_exact: that map (0: kept or not needed) */
  double flow_adjoint_exact_ms;     /* ... the interaction-region kernel and the cell sum of grad_perm_exact (0: none) */
  int64_t spgemm_path;             /* path of the last pfv_csr_matmul on this handle (csrc/csr_algebra.inc; tests): 0 none
                                      yet, 16 / 32 / 64 the sort in LDS with that many lanes per row (up to 64, up to 160,
                                      more products feeding the longest row), 1 the global radix sorts (a row fed by more
                                      than 4096 products, too little LDS, PFV_SPGEMM_GENERIC=1).  The host emulation
                                      reports the width the device would take */
  int64_t spgemm_lds_bytes;        /* ... dynamic LDS per workgroup of its sort-in-LDS launch (64 / width rows of
                                      8 capP + 8 capL + 8 (capP / 64 + 1) + 64 bytes each, rounded up to 16; capL the
                                      products of the longest row, capP the power of two from capL on); 0 on the global
                                      path.  Beyond 48 KiB the launch opts in to the larger LDS */
  double advdiff_adjoint_exact_ms;  /* last pfv_advdiff_adjoint / pfv_advdiff_adjoint_exact: the interaction-region passes
                                      and the cell sum of grad_conductivity_exact, HIP events read after the loop (0: none) */
  int64_t advdiff_adjoint_exact_passes; /* ... region-kernel launches: ceil(N / B) batches times the non-empty node
                                      classes (0: no step, a TPFA diffusion, or not asked for) */
  int64_t advdiff_adjoint_exact_batch; /* ... the B used: exact_batch (0: the default, 32) clipped to N (0: no region pass) */
  double transport_sorb_ms;        /* last pfv_transport_advance_sorb, all steps (HIP events) */
  int64_t transport_sorb_steps;    /* ... accepted steps */
  int64_t transport_sorb_core_iterations; /* ... nonlinear Jacobi iterations of the cyclic core, summed over the steps */
  int64_t transport_sorb_components; /* ... its k */
  int64_t topology_reference_path;   /* 1: the last topology rebuild ran the reference construction (PFV_TOPO_LEGACY=1, or
                                        an input the node-cooperative one hands over), 0: the node-cooperative one */
} pfv_stats;

pfv_status pfv_create(int device, pfv_ctx** out);
void pfv_destroy(pfv_ctx* h);
const char* pfv_last_error(pfv_ctx* h);
/* 1 if the library was built as the gfx950 HIP product, 0 for the host emulation build
 * that tests use to exercise the kernel logic without a GPU */
int pfv_is_device_build(void);

/* Grid arrays, the fields of pp.Grid the path reads (grids/grid.py:78-272):
 * cell_faces (CSC, Nf x Nc, data +-1, sorted indices), face_nodes (CSC, Nn x Nf),
 * nodes, face_normals, face_centers, cell_centers (3 x N), face_areas. */
pfv_status pfv_set_grid(pfv_ctx* h, int nd, int64_t nc, int64_t nf, int64_t nn,
                        const double* nodes, const int32_t* cf_indptr,
                        const int32_t* cf_indices, const int8_t* cf_sign,
                        const int32_t* fn_indptr, const int32_t* fn_indices,
                        const double* face_normals, const double* face_centers,
                        const double* cell_centers, const double* face_areas);

/* Discretization parameters (numerics/fv/mpfa.py:119-167): permeability as
 * SecondOrderTensor.values, shape (3,3,Nc) C-order; bc flags; Robin weight per face
 * (may be NULL = 1); eta scalar, or per-subface array (length = nnz(face_nodes), in
 * face_nodes CSC order) when eta_subface != NULL. */
pfv_status pfv_mpfa_set_params(pfv_ctx* h, const double* perm_33n, const uint8_t* bc_flags,
                               const double* robin_weight, double eta,
                               const double* eta_subface);

/* New permeability values only (same shape and order as above), everything else of pfv_mpfa_set_params kept: what
 * the step of a nonlinear / time-dependent model changes between two Mpfa.discretize calls (the reference reads
 * data[PARAMETERS][kw]["second_order_tensor"] afresh in every call, numerics/fv/mpfa.py:121-122).  perm_33n is host
 * memory, or device memory after pfv_set_vectors_on_device(h, 1) (copied device-to-device: the coefficient field of
 * a model that evaluates K on the GPU never crosses PCIe). */
pfv_status pfv_mpfa_set_permeability(pfv_ctx* h, const double* perm_33n);

/* Residual and Jacobian of the flow equation with a pressure-dependent permeability, on the device
 * (csrc/ad_flux.inc; the reference: AdTpfaFlux.diffusive_flux with an Mpfa base discretization,
 * models/constitutive_laws.py:1195-1336, 1580-1721): q = T_MPFA p + t_bnd bc + VS_MPFA g with the
 * matrices of the last pfv_mpfa_discretize (computed for K = K(p)), and the product rule
 * dq = T_MPFA dp + diag(w) dT_TPFA with the two-point derivative of the transmissibility.
 *   p         cell pressures (Nc)
 *   dk_dp     d K_rs(c) / d p_c, layout (3,3,Nc) like the permeability (NULL: K does not depend on p)
 *   bc_values per face (Dirichlet value / Neumann flux); vector_source nd per cell or NULL; source Nc or NULL
 *   flux_out  Nf values of q, or NULL
 * Leaves J = d(div q)/dp (pattern of PFV_MAT_SYSTEM) and -(div q - source) as the active system: pfv_solve
 * then returns the Newton increment; pfv_get_matrix(PFV_MAT_SYSTEM) / pfv_get_rhs copy them out.  With
 * PFV_AD_WANT_FLUX_JACOBIAN also dq/dp as PFV_MAT_FLUX_JACOBIAN (pattern of flux).  Vectors are host or
 * device memory as selected by pfv_set_vectors_on_device. */
#define PFV_AD_WANT_FLUX_JACOBIAN 1u
pfv_status pfv_mpfa_ad_flux_system(pfv_ctx* h, const double* p, const double* dk_dp, const double* bc_values,
                                   const double* vector_source, const double* source, double* flux_out,
                                   uint32_t flags);

/* Boundary conditions given per SUB-FACE (numerics/fv/mpfa.py:761-768): flags and Robin weights with
 * one entry per (face, node) pair in face_nodes CSC order (sorted indices), replacing the per-face
 * arrays of pfv_mpfa_set_params.  The following pfv_mpfa_discretize then keeps sub-face rows (and
 * sub-face columns of the boundary matrices) in matrices 0-3 -- no collapse to faces, traces not
 * averaged, Neumann data not divided by the number of face nodes (mpfa.py:1117-1125, 1516-1523) --
 * while matrices 4-5 keep face rows.  flags = NULL returns to per-face conditions. */
pfv_status pfv_mpfa_set_subface_bc(pfv_ctx* h, const uint8_t* bc_flags_sub, const double* robin_weight_sub);

/* Mpfa._flux_discretization (numerics/fv/mpfa.py:592-1156) on the device. */
pfv_status pfv_mpfa_discretize(pfv_ctx* h, uint32_t flags);

/* Two-point flux approximation, Tpfa.discretize (numerics/fv/tpfa.py:84-279): what the
 * reference's Mpfa delegates 1-D grids to (mpfa.py:690-712).  Uses the grid and the parameters
 * of pfv_mpfa_set_params (eta and Robin weights are not used); works for nd = 1, 2, 3.  Fills
 * matrices 0-5 with the patterns the reference stores (cell_faces pattern, diagonals);
 * vector_source_dim = ``ambient_dimension`` (number of vector-source components per cell). */
pfv_status pfv_tpfa_discretize(pfv_ctx* h, int vector_source_dim);

/* Differentiable two-point transmissibilities: the numerical core of
 * AdTpfaFlux.__transmissibility_matrix (models/constitutive_laws.py:1504-1578) on the half-face
 * geometry of DifferentiableTpfa (numerics/fv/tpfa.py:546-620), value and derivative in one pass
 * instead of two sparse products through the forward-AD machinery.  For every half-face
 * e = (cell c, face f, sign), in the order of the cell_faces entries given to pfv_set_grid (cell by
 * cell; the reference numbers its half-faces face by face, sps.find(sd.cell_faces), which only matters
 * for vectors indexed by half-face - the Jacobian below is the same matrix either way):
 *     t_e = d^T K_c n_f / |d|^2,  d = x_f - x_c        t_f = 1 / sum_{e of f} sgn_e / t_e
 *     t_face[f] = t_f                                   (Nf values)
 *     dt_dk[9 e + 3 r + s] = d t_f / d K_c[r][s] = t_f^2 sgn_e d_r n_s / (t_e^2 |d|^2)   (9 nnz(cell_faces))
 * i.e. row f(e), column 9 c(e) + 3 r + s of the Jacobian of t_f_full with respect to the reference's
 * k_c vector.  perm_33n: (3,3,Nc) C-order as in pfv_mpfa_set_params; needs only the grid.  The three
 * arrays follow pfv_set_vectors_on_device (host by default). */
pfv_status pfv_tpfa_transmissibility_ad(pfv_ctx* h, const double* perm_33n, double* t_face, double* dt_dk);

/* Partial (re)discretization: the node-list launch behind ``specified_cells / _faces /
 * _nodes`` (numerics/fv/mpfa.py:178-204, 466-508) and ``update_discretization``
 * (mpfa.py:510-590, _fvutils.py:1090-1257).  ``faces`` = the faces whose rows are to be
 * computed (the reference's ``active_faces``, _fvutils.py:1260-1462, computed by the host);
 * the interaction regions of their nodes are re-solved with the current parameters and
 * exactly these rows of the six matrices are rewritten.  keep_other_rows = 0: every other
 * row is zeroed (``specified_*`` semantics); 1: other rows keep the previous discretization
 * (update semantics; requires an earlier discretize on this handle). */
pfv_status pfv_mpfa_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces,
                                     const int32_t* faces, int keep_other_rows);

/* shape and nnz of a produced matrix */
pfv_status pfv_matrix_info(pfv_ctx* h, int which, int64_t* nrows, int64_t* ncols,
                           int64_t* nnz);
/* copy a matrix to caller-allocated CSR arrays (indptr nrows+1, indices nnz, data nnz);
 * any pointer may be NULL to skip that array */
pfv_status pfv_get_matrix(pfv_ctx* h, int which, int32_t* indptr, int32_t* indices,
                          double* data);
/* the same for a list of rows only (gathered on the device, one copy): what a caller that slices
 * `data[DISCRETIZATION_MATRICES][kw]["flux"][faces]` needs instead of the whole matrix (21.6 GB for the
 * six matrices of a 2 M-cell grid).  out_indptr has n_rows + 1 entries (row i of the output = row rows[i]);
 * call once with out_indices = out_data = NULL to learn the sizes, then again with the arrays. */
/* free / total bytes of the handle's device (free includes the blocks parked in the handle's own cache);
 * -1 / -1 from the host-emulation build.  The host mirror checks its footprint estimate against it before
 * the first discretization of a grid (the reference's peak-memory estimate: mpfa.py:1315-1355). */
pfv_status pfv_device_memory(pfv_ctx* h, int64_t* free_bytes, int64_t* total_bytes);
/* Page-locked host memory for the arrays the copy-out calls fill (pfv_get_matrix, pfv_get_rhs, pfv_solve): into such a
 * buffer the device writes over PCIe directly (~50 GB/s), into pageable memory the runtime stages the copy (23 GB/s
 * measured) and the freshly allocated pages fault in first (the "eager" operator path moved 23 GB at 6 GB/s that
 * way).  The host mirror keeps the blocks in a pool and hands them to numpy (porepy_amd/_lib.py: PinnedPool), so that
 * the matrices of the next time step land in the blocks the previous ones gave back.  Host emulation: malloc / free.
 * (The reference's matrices are ordinary scipy arrays: fv_elliptic.py:67-112 -- so are these, only their memory
 * comes from here.) */
pfv_status pfv_host_alloc(size_t bytes, void** out);
void pfv_host_free(void* p);
/* number of unknowns of the system pfv_solve / pfv_get_rhs operate on (0: nothing assembled): the length of
 * the arrays those calls write */
pfv_status pfv_active_size(pfv_ctx* h, int64_t* n);
pfv_status pfv_get_matrix_rows(pfv_ctx* h, int which, int64_t n_rows, const int32_t* rows, int32_t* out_indptr,
                               int32_t* out_indices, double* out_data);

/* FVElliptic.assemble_matrix_rhs (numerics/fv/fv_elliptic.py:67-112):
 * A = div @ flux, b = -div @ bound_flux @ bc_values - div @ vector_source @ g + source.
 * vector_source (Nc*nd) and source (Nc) may be NULL.  Results stay on the device. */
pfv_status pfv_mpfa_assemble(pfv_ctx* h, const double* bc_values, const double* vector_source,
                             const double* source);
pfv_status pfv_get_rhs(pfv_ctx* h, double* b);

/* y = M x for a produced matrix; host vectors (testing / flux post-processing) */
pfv_status pfv_spmv(pfv_ctx* h, int which, const double* x, double* y);

/* ---- Biot: coupling terms of the poro-elastic discretization (numerics/fv/biot.py:247-1135),
 * computed from the same interaction-region inverse as MPSA.  One set of five matrices per
 * coupling tensor ("scalar_vector_mappings" of the reference: Biot's alpha, thermal expansion...). */
enum {
  PFV_BIOT_SCALAR_GRADIENT = 0,                 /* (nd Nf x Nc)  */
  PFV_BIOT_DISPLACEMENT_DIVERGENCE = 1,         /* (Nc x nd Nc)  */
  PFV_BIOT_BOUNDARY_DISPLACEMENT_DIVERGENCE = 2, /* (Nc x nd Nf)  */
  PFV_BIOT_CONSISTENCY = 3,                     /* (Nc x Nc), "mpsa_consistency" */
  PFV_BIOT_BOUND_DISPLACEMENT_PRESSURE = 4,     /* (nd Nf x Nc)  */
  PFV_BIOT_NUM_TERMS = 5
};
/* coupling tensors as SecondOrderTensor.values, shape (nalpha, 3, 3, Nc) C-order; nalpha = 0
 * switches the coupling terms off.  Needs the grid and pfv_mpsa_set_params. */
pfv_status pfv_biot_set_alphas(pfv_ctx* h, int nalpha, const double* alpha_k33n);
/* Partial discretization / update of the coupling terms (biot.py:151-245 update_discretization,
 * :326-345 specified_cells / faces / nodes): the interaction regions of the nodes of `faces` are
 * recomputed; face rows (stress, bound_stress, traces, scalar_gradient, bound_displacement_pressure)
 * of `faces` and cell rows (displacement_divergence, boundary_displacement_divergence, consistency) of
 * `cells` are rewritten - the caller passes cells all of whose nodes are among the nodes of `faces`,
 * so that their rows are complete.  keep_other_rows = 0: every other row becomes zero (partial
 * discretization); 1: they keep their values (update). */
pfv_status pfv_biot_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces, const int32_t* faces,
                                     int64_t n_cells, const int32_t* cells, int keep_other_rows);

/* Biot._local_discretization (biot.py:714-878): pfv_mpsa_discretize plus the coupling terms */
pfv_status pfv_biot_discretize(pfv_ctx* h, uint32_t flags);
pfv_status pfv_biot_matrix_info(pfv_ctx* h, int term, int64_t* nrows, int64_t* ncols, int64_t* nnz);
pfv_status pfv_biot_get_matrix(pfv_ctx* h, int term, int key, int32_t* indptr, int32_t* indices,
                               double* data);

/* Hand an assembled system to the device solver: the caller of the hot path one level up,
 * SolutionStrategy.solve_linear_system (models/solution_strategy.py:830-884), holds the global
 * Jacobian as a scipy CSR matrix and the residual as a numpy vector.  CSR arrays (int32, any
 * column order inside a row) and rhs are copied to the device; every row needs a non-zero
 * diagonal entry (Jacobi preconditioner) or PFV_ERR_UNSUPPORTED is returned.  pfv_solve then
 * operates on this system; needs no grid. */
pfv_status pfv_set_system(pfv_ctx* h, int64_t n, const int32_t* indptr, const int32_t* indices,
                          const double* data, const double* rhs);

/* Periodic faces (Grid.set_periodic_map, grids/grid.py:879-911; SubcellTopology merges the right
 * sub-faces and nodes into the left ones, numerics/fv/_fvutils.py:91-137; Tpfa pairs the cells,
 * numerics/fv/tpfa.py:114-262).  The host passes the *merged* grid to pfv_set_grid (the right cell lists
 * the left face, right nodes renamed to left nodes, right faces left without cells and nodes;
 * porepy_amd/periodic.py) and tells here which side of a merged face is displaced: for every face f,
 * native_cell[f] = the cell that sees the face where it is (-1: not a periodic face) and
 * shift[3][Nf] (SoA) = x_f(left) - x_f(right); every other cell of f sees the face centre at
 * face_centers[f] - shift[f].  Call after pfv_set_grid (which clears it); NULL, NULL clears. */
pfv_status pfv_set_periodic(pfv_ctx* h, const int32_t* native_cell, const double* shift);

/* Where the vector arguments of pfv_mpfa_assemble (bc_values, vector_source, source),
 * pfv_mpsa_assemble (bc_values, source) and pfv_solve (x0, x) live: 0 (default) host memory, as the
 * reference's numpy arrays (fv_elliptic.py:67-112); 1 device memory of this handle's GPU - models
 * that keep iterating on the device skip PCIe altogether.  Device buffers must be complete on the
 * handle's stream (see pfv_set_stream) when the call is made; pfv_solve returns after x is written. */
pfv_status pfv_set_vectors_on_device(pfv_ctx* h, int on);

/* Select the preconditioner of the following pfv_solve calls on this handle. */
pfv_status pfv_set_preconditioner(pfv_ctx* h, int kind);

/* PFV_PRECOND_SWEEP (csrc/sweep.inc): z = M^-1 r by one substitution in flow order.  The order is built on the device
 * from the face flux q of the active transport (PFV_MAT_TRANSPORT_SYSTEM) or advection-diffusion
 * (PFV_MAT_ADVDIFF_SYSTEM) system: an interior face with q != 0 (and not NaN) is an edge upstream cell -> downstream
 * cell.  A forward peel gives every cell its longest upstream path as level; a backward peel of what is left takes the
 * cells without outflow into the rest, which get the highest levels; what both leave is the cyclic core, one level
 * between the two (no core: the flux graph is acyclic).  M holds the diagonal of S and the entries S[i,j] with
 * level[j] < level[i].  For the transport system of an acyclic flux M = S: pfv_solve and every step of
 * pfv_transport_advance then do one sweep and one true-residual check instead of a Krylov loop (iterations = 1;
 * should the check fail, GMRES preconditioned by the sweep goes on from there).  Otherwise the sweep preconditions the
 * requested method.  Any other active system, pfv_solve_sharded and pfv_amg_setup*: PFV_ERR_UNSUPPORTED.  The order is
 * built by the first solve that needs it and kept until an assembly brings a flux with other edges (or pfv_set_grid).
 * PFV_SWEEP_MERGE=0: one launch per level instead of runs of small levels in single-workgroup launches.
 *
 * pfv_sweep_info (tests): info = {cells, levels, core cells, index of the core level or -1}; level (Nc) and order (Nc:
 * the cells sorted by level, ascending inside a level) in the caller's cell numbering, either may be NULL.  It only
 * copies out.  PFV_ERR_ARGUMENT when no order has been built. */
pfv_status pfv_sweep_info(pfv_ctx* h, int64_t info[4], int32_t* level, int32_t* order);

/* Near-null space of PFV_PRECOND_AMG_NNS for the active system: B is a host array of n x k values, column-major, in
 * the caller's numbering of the n unknowns (bs per cell, cell-major / component-minor).  B == NULL: the rigid-body
 * modes of the handle's grid, built on the device from its cell centres -- 2-D: 2 translations + the rotation (k = 3),
 * 3-D: 3 translations + 3 rotations (k = 6); only for the assembled mechanics system (bs = nd).  k = 0 clears the modes.
 * k > 8: PFV_ERR_UNSUPPORTED.  The modes follow the renumbering pfv_solve applies to grid systems.  The hierarchy of
 * PFV_PRECOND_AMG_NNS is kept apart from the one of PFV_PRECOND_AMG; it has no sharded form (pfv_amg_setup,
 * pfv_amg_setup_sharded and pfv_solve_sharded with it selected return PFV_ERR_UNSUPPORTED). */
pfv_status pfv_set_near_null_space(pfv_ctx* h, int bs, int k, const double* B);

/* Introspection of the PFV_PRECOND_AMG_NNS hierarchy built by the last pfv_solve (tests): for level `level`,
 * info[6] = {rows n_l, block size bs_l, modes k, aggregates (0 on the coarsest level), nnz of A_l, levels}; then, each
 * optional (NULL: skipped): agg [n_l / bs_l] cell -> aggregate, P [n_l][k] tentative prolongator (row-major),
 * B [n_l][k] the level's near-null space, Bc [aggregates * k][k] the next level's (R of the QR per aggregate),
 * A_l as CSR (indptr [n_l + 1], indices and val [nnz], FP64).  Level 0 is in the numbering the solve worked in. */
pfv_status pfv_amg_nns_level(pfv_ctx* h, int level, int64_t* info, int32_t* agg, double* P, double* B, double* Bc,
                             int32_t* indptr, int32_t* indices, double* val);

/* One cycle of that hierarchy on device vectors of its n_0 rows (tests): d_z = cycle(level 0, d_r), d_r != d_z.  The
 * twin of pfv_amg_apply_device: it only runs the cycle the solve runs, on the hierarchy's own scratch vectors, and
 * changes nothing a later solve depends on.  The vectors are in the numbering of the system the hierarchy was built
 * for: the caller's for a user system, the numbering the solve worked in (the renumbering along the cell order, when
 * pfv_solve applied it) for a grid system.  PFV_ERR_ARGUMENT without a valid hierarchy, as pfv_amg_nns_level. */
pfv_status pfv_amg_nns_apply_device(pfv_ctx* h, const double* d_r, double* d_z);

/* Introspection of the plain aggregation hierarchy (PFV_PRECOND_AMG) that was set up last on this handle, by
 * pfv_amg_setup or by a pfv_solve with PFV_PRECOND_AMG (tests).  It only copies data out: no kernel, launch or buffer
 * of the setup or the cycle depends on it.  Numbering: the hierarchy of pfv_amg_setup is built on the active system as
 * it is, so its level 0 -- and the vectors of pfv_amg_apply_device -- are in the CALLER's numbering of the unknowns,
 * for grid systems too (cell-major / component-minor); the hierarchy of a pfv_solve of a grid system is in the
 * numbering the solve worked in (the renumbering along the cell order, when pfv_solve applied it).
 * info[24] = { 0 rows n_l, 1 block size, 2 levels, 3 coarse cells (0 on the coarsest level), 4 nnz of A_l, 5 nnz of the
 *   operator, 6 nnz of the system (level 0, else 0), 7 the cycle's products read the FP32 copy of the operator's values,
 *   8 path bits of this level (1 residual inside the restriction, 2 prolongation inside the post-smoothing of a small
 *   level, 4 prolongation inside the post-smoothing product of a larger level, 8 visited twice by its parent, 16 visits
 *   the next level twice, 32 ... with residual and first smoothing step in one product, 64 coarsest level by the dense
 *   inverse, 128 coarsest level by Jacobi sweeps), 9 dense inverse in use, 10 gamma, 11 gamma_levels, 12 fuse_rows,
 *   13 fuse_cycle, 14 the last setup kept its aggregate maps (values-only branch), 15 filter_level0, 16 restrict_lanes,
 *   17 the level's products go through an SpMV window, 18 mptr / mem are kept, 19 largest number of entries gathered
 *   into one coarse row by the Galerkin products of the last setup, 20 kAmgDenseMax, 21 kGalEpl, 22 kGalMaxMembers,
 *   23 kAmgWTopRows };  params[4] = { omega_l, alpha, filter theta, rho_l (0: not estimated) }.
 * Each of the following is optional (NULL: skipped); CSR triples are indptr [n_l + 1], indices and FP64 values [nnz]:
 *   sys_*  level 0 only: the matrix the setup was given (the leading block for n_own < n), before the strength filter;
 *   a_*    A_l, the matrix the level was coarsened from (level 0: the strength-filtered copy when the filter is on);
 *   op_*   the operator the cycle's products read on the level (level 0: the filtered copy when filter_level0 is set,
 *          else the system); the products read its values rounded to FP32 when info[7] is set;
 *   dinv [n_l] the smoother's inverse diagonal after the row safeguard; agg [n_l / bs] cell -> coarse cell,
 *   mptr [coarse cells + 1] and mem [n_l / bs] the members of every coarse cell (not on the coarsest level);
 *   dense [n_l * n_l] row-major inverse of the coarsest matrix (coarsest level, info[9] set).
 * PFV_ERR_ARGUMENT: no hierarchy or level out of range; PFV_ERR_UNSUPPORTED: the coupled hierarchy of a sharded solve. */
pfv_status pfv_amg_level(pfv_ctx* h, int level, int64_t* info, double* params, int32_t* sys_indptr, int32_t* sys_indices,
                         double* sys_val, int32_t* a_indptr, int32_t* a_indices, double* a_val, int32_t* op_indptr,
                         int32_t* op_indices, double* op_val, double* dinv, int32_t* agg, int32_t* mptr, int32_t* mem,
                         double* dense);

/* Right-hand side level `level` >= 1 of that hierarchy worked on in its last first visit (tests): out [n_l] on the host,
 * the restricted residual of the level above as the last cycle left it.  Errors as pfv_amg_level. */
pfv_status pfv_amg_level_rhs(pfv_ctx* h, int level, double* out);

/* Block preconditioner (PFV_PRECOND_BLOCK) for the coupled Jacobians of mixed-dimensional / multi-physics models
 * that the reference solves directly (models/solution_strategy.py:830-884; mortar coupling
 * models/constitutive_laws.py:987-1000): the unknowns of the system given to pfv_set_system are grouped in
 * n_blocks contiguous blocks [block_ptr[k], block_ptr[k+1]) -- one per (variable, subdomain or interface) -- and
 * the preconditioner is the block lower-triangular part of A, every diagonal block solved by one cycle of its own
 * aggregation-AMG hierarchy (blocks of at most 1024 rows: exactly, by the dense inverse of the block as given -- the
 * strength filter of the hierarchies, PFV_AMG_FILTER_PERMIL, does not touch them).  gauss_seidel = 0: block
 * Jacobi.  The coupling term of block k sums every stored entry of its rows whose column lies left of the block,
 * whatever the order of the columns inside a row (as pfv_set_system accepts them); rows stored with ascending columns
 * give the same sums, entry for entry in the same order.  Every diagonal entry must be non-zero: systems whose
 * equations are ordered differently from their unknowns are row-permuted first (host side:
 * porepy_amd.solvers.match_rows).  Selects PFV_PRECOND_BLOCK; the blocks are (re)built by the next pfv_solve. */
pfv_status pfv_set_block_preconditioner(pfv_ctx* h, int64_t n_blocks, const int64_t* block_ptr, int gauss_seidel);

/* Jacobi-preconditioned Krylov solve of A x = b on the device (stand-in for
 * SolutionStrategy.solve_linear_system, models/solution_strategy.py:830-884).
 * x0 may be NULL (zero start); x receives Nc values. */
pfv_status pfv_solve(pfv_ctx* h, int method, double rtol, int maxit, int restart,
                     const double* x0, double* x, pfv_solve_info* info);

/* ---- MPSA-W (numerics/fv/mpsa.py): same grid, vector unknowns ------------------------------
 * stiffness: FourthOrderTensor.values, shape (9,9,Nc) C-order (params/tensor.py:300-349);
 * bc_dir_bits / bc_neu_bits: per face, bit a set if component a is Dirichlet / Neumann
 * (BoundaryConditionVectorial.is_dir / is_neu, params/bc.py:222-322; Cartesian basis, no Robin);
 * cell_volumes: Grid.cell_volumes (Nc), the weights of the node average (mpsa.py:1619-1640);
 * eta as in pfv_mpfa_set_params (scalar). */
pfv_status pfv_mpsa_set_params(pfv_ctx* h, const double* stiffness_99n, const double* cell_volumes,
                               const uint8_t* bc_dir_bits, const uint8_t* bc_neu_bits, double eta);
/* Continuity points per sub-face for MPSA (`mpsa_eta` given as an array of SubcellTopology.num_subfno_unique values,
 * numerics/fv/mpsa.py:293-303, 647-652; _fvutils.py:222-277): eta_subface[s] for sub-face s = position of the (face,
 * node) pair in the face_nodes CSC arrays, used as given also on the boundary.  Call after pfv_mpsa_set_params (which
 * clears it); NULL removes it. */
pfv_status pfv_mpsa_set_subface_eta(pfv_ctx* h, const double* eta_subface);
/* `reconstruction_eta` (numerics/fv/mpsa.py:185, 757-761, _reconstruct_displacement :1187-1266): the displacement
 * traces (bound_displacement_cell / bound_displacement_face) are reconstructed at x_f + hf_eta (x_v - x_f) from the
 * sub-cell gradients, averaged over the two sides of the sub-face, instead of at the continuity points (a scalar: 0
 * on boundary faces, as the reference's distance routine does).  on = 0 switches back.  After pfv_mpsa_set_params
 * (which clears it).  Not combined with the Biot coupling terms (PFV_ERR_UNSUPPORTED). */
pfv_status pfv_mpsa_set_reconstruction_eta(pfv_ctx* h, int on, double hf_eta);
/* the same with one value per sub-face (compute_dist_face_cell with an array, numerics/fv/_fvutils.py:222-277: used as
 * given, also on the boundary), sub-faces in the order of the sorted face_nodes CSC arrays; NULL switches the
 * reconstruction points back to the continuity points. */
pfv_status pfv_mpsa_set_reconstruction_eta_subface(pfv_ctx* h, const double* hf_eta_subface);
/* Robin conditions of the vectorial boundary condition (BoundaryConditionVectorial.is_rob,
 * .robin_weight, params/bc.py:222-322; rows of numerics/fv/mpsa.py:1381-1459): bit c of
 * bc_rob_bits[f] = component c of face f is Robin; robin_weight_ddn = weights W[i][a][f], shape
 * (nd, nd, Nf) C-order (NULL = identity).  Call after pfv_mpsa_set_params (which clears them);
 * bc_rob_bits = NULL removes them. */
pfv_status pfv_mpsa_set_robin(pfv_ctx* h, const uint8_t* bc_rob_bits, const double* robin_weight_ddn);
/* face-wise basis in which the boundary conditions are given (BoundaryConditionVectorial.basis,
 * shape (nd, nd, Nf) C-order; row k = the k-th direction); NULL = Cartesian.  Call after
 * pfv_mpsa_set_params (which resets it). */
pfv_status pfv_mpsa_set_basis(pfv_ctx* h, const double* basis_ddn);

/* Conditions per SUB-FACE (numerics/fv/mpsa.py:712-720: a BoundaryConditionVectorial with one entry per sub-face;
 * :752-754, 780-781 the outputs; :1127-1138 Neumann / Robin data integrated over the sub-face, not divided by
 * #nodes).  Arrays with one entry per sub-face in the order of the SORTED face_nodes CSC arrays: component bit
 * masks as in pfv_mpsa_set_params, optional Robin flags and weights (nd, nd, Nsf) C-order (NULL = identity).
 * After this call pfv_mpsa_discretize fills
 *   PFV_MAT_STRESS                   (nd Nsf x nd Nc)    one row block per sub-face
 *   PFV_MAT_BOUND_STRESS             (nd Nsf x nd Nsf)
 *   PFV_MAT_BOUND_DISPLACEMENT_CELL  (nd Nf  x nd Nc)    as with conditions per face
 *   PFV_MAT_BOUND_DISPLACEMENT_FACE  (nd Nf  x nd Nsf)
 * and pfv_mpsa_assemble refuses (the caller collapses the sub-face rows first, as with the reference).
 * bc_dir_bits_sub = NULL returns to conditions per face; pfv_mpsa_set_params resets it.  Not combined with
 * Biot coupling terms or partial updates; a basis comes per sub-face too (pfv_mpsa_set_subface_basis). */
pfv_status pfv_mpsa_set_subface_bc(pfv_ctx* h, const uint8_t* bc_dir_bits_sub, const uint8_t* bc_neu_bits_sub,
                                   const uint8_t* bc_rob_bits_sub, const double* robin_weight_dds);
/* the basis of conditions per sub-face (the .basis of a BoundaryConditionVectorial with one entry per sub-face,
 * numerics/fv/_fvutils.py:836-852 through ExcludeBoundaries.basis_matrix): shape (nd, nd, Nsf) C-order, sub-faces in
 * the order of the sorted face_nodes CSC arrays; NULL = Cartesian.  Call after pfv_mpsa_set_subface_bc (which
 * resets it). */
pfv_status pfv_mpsa_set_subface_basis(pfv_ctx* h, const double* basis_dds);

/* Mpsa._stress_discretization (numerics/fv/mpsa.py:531-782) on the device; fills matrices 7-10 */
pfv_status pfv_mpsa_discretize(pfv_ctx* h, uint32_t flags);

/* Partial MPSA (re)discretization, same contract as pfv_mpfa_discretize_faces
 * (numerics/fv/mpsa.py:196-216, 383-416 and Mpsa.update_discretization :418-487): the
 * interaction regions around the listed faces are re-solved, the nd rows of each listed face
 * are rewritten in the four matrices, the other rows are zeroed (keep_other_rows = 0) or kept. */
pfv_status pfv_mpsa_discretize_faces(pfv_ctx* h, uint32_t flags, int64_t n_faces,
                                     const int32_t* faces, int keep_other_rows);
/* Mpsa.assemble_matrix_rhs (mpsa.py:486-529): A = div_nd @ stress,
 * b = -div_nd @ bound_stress @ bc_values + source; bc_values has nd*Nf entries ((nd,Nf) raveled
 * column-major), source nd*Nc or NULL.  Makes the mechanics system the one pfv_solve works on
 * (pfv_mpfa_assemble switches back to the flow system). */
pfv_status pfv_mpsa_assemble(pfv_ctx* h, const double* bc_values, const double* source);

/* ---- Upwind advection and the transport step on the device (csrc/upwind.inc; numerics/fv/upwind.py) ----------
 * The chain discretize flow -> solve -> Darcy flux -> upwind -> transport step without leaving the device.  Vectors
 * (p, bc_values, vector_source, q, accumulation, c_old, source, c and the outputs) are host or device memory as
 * selected by pfv_set_vectors_on_device; the flag array is host memory.  Periodic grids, conditions per sub-face and
 * the sharded solve are not covered (PFV_ERR_UNSUPPORTED).  pfv_set_grid clears all of it.
 *
 * Face flux q = flux p + bound_flux bc_values (+ vector_source g) from the MPFA / TPFA matrices on the handle, each
 * row summed in stored order (flux, then bound_flux, then vector_source).  The result stays on the handle as the
 * resident face flux; q_out (Nf, may be NULL) receives a copy. */
pfv_status pfv_mpfa_face_flux(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                              double* q_out);
/* Boundary conditions of the transport keyword: Nf bytes of PFV_BC_* bits; NULL = Dirichlet on every boundary face
 * (the reference's default, upwind.py:232-238). */
pfv_status pfv_upwind_set_bc(pfv_ctx* h, const uint8_t* bc_flags);
/* Upwind.discretize for the face flux q (Nf; NULL = the resident face flux): fills PFV_MAT_UPWIND,
 * PFV_MAT_UPWIND_RHS_DIR and PFV_MAT_UPWIND_RHS_NEU with the patterns the reference stores (num_components = k: a
 * full k x k block per entry, as scipy's kron with eye(k) leaves it -- zeros off the block diagonal stored).  The upstream side
 * follows numpy's sign(q) >= 0: +0 and -0 count as positive, NaN as negative.  A boundary face that is neither
 * Dirichlet nor Neumann and has inflow has no upstream cell: PFV_ERR_ARGUMENT (the reference: ValueError). */
pfv_status pfv_upwind_discretize(pfv_ctx* h, const double* q, int num_components);
/* Upwind.assemble_matrix_rhs, fused: A = div diag(q) U + diag(accumulation) as PFV_MAT_TRANSPORT_SYSTEM on the
 * pattern {cell, its face neighbours} (explicit zeros where the reference stores nothing), and the boundary part of
 * the flux divergence b_ref = div (rhs_neu + rhs_dir diag(q)) bc_values, which is what the reference returns as
 * "rhs": the balance reads accumulation o (c - c_old) + A c + b_ref = source.  (A, r) with
 * r = accumulation o c_old - b_ref + source become the active system of pfv_solve.  q = NULL: the flux of the
 * discretization; accumulation, c_old, source (Nc each) and bound_rhs_out (Nc, receives b_ref) may be NULL.
 * c_old without accumulation has nothing to multiply and is ignored.
 * num_components must be 1. */
pfv_status pfv_upwind_assemble(pfv_ctx* h, const double* q, const double* bc_values, const double* accumulation,
                               const double* c_old, const double* source, double* bound_rhs_out);
/* n_steps implicit Euler steps with the system of pfv_upwind_assemble: per step r = accumulation o c - b_ref + source
 * on the device, Jacobi-preconditioned solve (method: PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES; the matrix is not
 * symmetric) started from c, c <- x.  BiCGStab breaks down (rho = 0, the residual turns NaN) when the first residual
 * sits in cells nothing flows back into -- injection into a field at rest: the matrix of an acyclic flow is triangular;
 * such a step is solved again with GMRES from the kept state and counted in pfv_stats.transport_gmres_retries.
 * c holds c_0 on entry and the last computed state on return.  Stops at the first
 * step that does not converge (PFV_ERR_NOT_CONVERGED; steps_done counts the converged ones).  last (may be NULL)
 * receives the info of the last solve.  With PFV_PRECOND_SWEEP selected on the handle the steps use it (any other
 * selection: Jacobi, as ever): for an acyclic flux every step is one sweep and one residual check
 * (pfv_stats.sweep_direct_steps), and the order is built by the first step. */
pfv_status pfv_transport_advance(pfv_ctx* h, int n_steps, int method, double rtol, int maxit, double* c,
                                 int32_t* steps_done, pfv_solve_info* last);
/* n_steps implicit Euler steps of n_comp (1 .. 64, else PFV_ERR_ARGUMENT) quantities on one flux: component a solves
 * (diag(accumulation[a]) + A) c[a] = accumulation[a] o c[a] - b_ref(bc_values[a]) + source[a] with A = div diag(q) U of
 * the one-component discretization on the handle (pfv_upwind_discretize with num_components = 1).  All arrays are
 * component-major: bc_values [n_comp][Nf], accumulation, source (may be NULL) and c (in and out) [n_comp][Nc]; q (Nf)
 * NULL = the flux of the discretization.  On the device the vectors are cell-major and interleaved, v[i * n_comp + a];
 * the transposition happens there.  The call does not need pfv_upwind_assemble and leaves no transport system behind:
 * afterwards pfv_solve asks for an assembly, as after pfv_upwind_set_bc; the flow order stays.
 *   With PFV_PRECOND_SWEEP selected and an acyclic flux, every step is one right-hand side, one sweep that carries
 * all components (the matrix and the levels are read once, csrc/sweep.inc: sweep_apply_multi), one residual check of
 * all of them and one host read; last[a].iterations = 1.  A component whose check fails is stepped from the state at
 * the start of the step by pfv_upwind_assemble + pfv_transport_advance on its own arrays, the others keep their
 * result.  With any other preconditioner, or a cyclic core, every component is stepped that way.
 *   A zero or NaN diagonal A[i,i] + accumulation[a][i]: PFV_ERR_UNSUPPORTED naming the first such row and its first
 * such component.  c holds the state after the last step completed by all components, steps_done that number of
 * steps; last (n_comp entries, may be NULL) the info of every component's last solve.  pfv_stats:
 * transport_multi_*, sweep_levels / sweep_launches / sweep_order_ms as after pfv_transport_advance. */
pfv_status pfv_transport_advance_multi(pfv_ctx* h, const double* q, int n_comp, const double* bc_values,
                                       const double* accumulation, const double* source, int n_steps, int method,
                                       double rtol, int maxit, double* c, int32_t* steps_done, pfv_solve_info* last);
/* n_steps implicit upwind steps of a saturation s that moves with q f(s) (csrc/sweep.inc: sweep_apply_nl).  Per cell
 *     acc_i (s_i - s_old_i) + (A_ii + sink_i) f(s_i) + sum_{j != i} A_ij f(s_j) + b_ref_i = source_i
 * with A = div diag(q) U of the one-component discretization on the handle (pfv_upwind_discretize with
 * num_components = 1; no pfv_upwind_assemble is needed) and b_ref = div (rhs_neu bc + rhs_dir diag(q) f(bc)): a Dirichlet
 * inflow value is a saturation, a Neumann value a flux of the transported phase, values on outflow faces are not read.
 * In flow order every cell is one scalar monotone root-finding given its upstream cells: no Jacobian, no Krylov loop.
 * The cells of a cyclic core are iterated by nonlinear Jacobi until ||F_core|| <= rtol ||rhs|| / 2 or maxit iterations;
 * a step is accepted when ||F(s)|| <= rtol ||rhs|| over all rows, rhs = acc o s_old - b_ref + source.
 *   fluxfn_kind / fluxfn_params / n_params: a PFV_FLUXFN_* and its parameters (host memory).  q (Nf): NULL = the flux
 * of the discretization.  accumulation (Nc) must be positive; source and sink (Nc, sink >= 0: a production rate that
 * removes fluid at the cell's own f(s_i)) may be NULL.  s (Nc) holds the state in [0, 1] on entry and the state after
 * the last accepted step on return, steps_done that number of steps.  last (may be NULL): iterations = 1 for an acyclic
 * flux, else the core iterations of the last step; rel_residual the measured ||F|| / ||rhs||.
 *   PFV_ERR_ARGUMENT (the text names the first offender): no discretization or num_components != 1; an unknown kind,
 * a wrong n_params, Corey parameters with a negative residual saturation, s_wr + s_nr >= 1, an exponent or viscosity
 * <= 0; a table that decreases or is not finite; accumulation <= 0 or NaN; a negative sink; s or a Dirichlet inflow
 * value outside [0, 1]; a boundary face with inflow that is neither Dirichlet nor Neumann; a step whose solution
 * leaves [0, 1] (the text holds the step and the lowest such cell; s is the state before that step).
 * PFV_ERR_NOT_CONVERGED: the core iteration or the acceptance check of a step failed; s is the state before it.
 * PFV_ERR_UNSUPPORTED: periodic grids, conditions per sub-face, the sharded solve.
 *   The flow order is built if the handle has none for this flux, whatever preconditioner is selected, and stays under
 * the rules of pfv_transport_advance; the selected preconditioner and the flow system are left alone; no transport
 * system is left behind (pfv_solve asks for an assembly).  pfv_stats: transport_nl_*, sweep_levels / sweep_core_cells /
 * sweep_launches / sweep_order_ms. */
pfv_status pfv_transport_advance_nl(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                    int n_params, const double* bc_values, const double* accumulation,
                                    const double* source, const double* sink, int n_steps, double rtol, int maxit,
                                    double* s, int32_t* steps_done, pfv_solve_info* last);
/* The same steps with k (1 .. 64, else PFV_ERR_ARGUMENT) components carried by the transported phase: salinity, a
 * polymer, a tracer that marks injected water, the water's heat content.  c_a is the amount of component a per unit
 * volume of the phase.  After s_i and phi_i = f(s_i) of the step are known, component a solves, with o_i = A_ii + sink_i,
 *     (acc_i s_i + ads_ai) c_ai + o_i phi_i c_ai + sum_{j != i} A_ij phi_j c_aj
 *         = (acc_i s_old_i + ads_ai) c_old_ai - b_ref_ai + src_ai
 *     b_ref_a = div (rhs_neu cbc_a + rhs_dir diag(q) (f(bc) o cbc_a)):
 * on a Dirichlet inflow face c_bc_values[a] is the concentration in the entering phase (the saturation there is still
 * bc_values through f), on a Neumann face the component's flux; values on outflow faces are not read.  c_source[a] is a
 * mass rate of the component; the sink removes it at sink_i phi_i c_ai; sorption[a] >= 0 is a linear sorption capacity
 * that does not scale with s (the retardation of pfv_transport_advance_multi).  In flow order the row is one division
 * once s_i is known, in the launches of the saturation (csrc/sweep.inc: sweep_row_nlc): pfv_stats.sweep_launches is that
 * of pfv_transport_advance_nl, and s is, bit for bit, what that call computes from the same arguments.  A row whose
 * diagonal acc_i s_i + ads_ai + o_i phi_i is zero (a dry cell without sorption) keeps c_old_ai.  The cells of a cyclic
 * core iterate s and c jointly; the core has settled when ||F_core|| <= rtol ||rhs|| / 2 holds for the saturation and
 * for every component with its own rhs_a.
 *   c_bc_values [k][Nf], sorption and c_source ([k][Nc], each may be NULL) and c ([k][Nc], in and out) are
 * component-major; on the device the vectors are cell-major and interleaved, v[i * k + a].  (k + 1) max(Nc, Nf) must stay
 * below 2^31 (PFV_ERR_UNSUPPORTED).  A step is accepted only if the saturation and every component satisfy
 * ||F|| <= rtol ||rhs||, 0 <= 0 included (a component that is absent everywhere is valid); one host read per step brings
 * all 2 (k + 1) norms and the status words.  A refused step returns s and c of the step's start, steps_done and
 * PFV_ERR_NOT_CONVERGED; a step that leaves [0, 1] PFV_ERR_ARGUMENT as above.  There is no per-component fallback: the
 * matrix of a component changes with s in every step, so no assembled linear system exists to fall back to.
 *   PFV_ERR_ARGUMENT beyond those of pfv_transport_advance_nl: a negative or NaN sorption, a non-finite c, a non-finite
 * c_bc_values on a Dirichlet inflow or Neumann face (the text names the lowest cell or face and its lowest component).
 * last (k + 1 entries, may be NULL): the saturation first, then the components.  The handle rules are those of
 * pfv_transport_advance_nl; pfv_stats: transport_nl_* (transport_nl_components = k) and the sweep_* fields. */
pfv_status pfv_transport_advance_nl_multi(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                          int n_params, const double* bc_values, const double* accumulation,
                                          const double* source, const double* sink, int k, const double* c_bc_values,
                                          const double* sorption, const double* c_source, int n_steps, double rtol,
                                          int maxit, double* s, double* c, int32_t* steps_done, pfv_solve_info* last);

/* n_steps implicit Euler steps of k (1 .. 8, else PFV_ERR_ARGUMENT) COUPLED components on one flux: a decay chain,
 * reversible first-order kinetics, kinetic sorption or mobile-immobile exchange, biodegradation with a yield.  Per cell i
 * and component a
 *     acc_ia (c_ia - c_old_ia) + w_a [sum_j A_ij c_ja + b_ref_ia] + rho_i sum_b K_ab c_ib = src_ia
 *     b_ref_a = div (rhs_neu + rhs_dir diag(q)) bc_values[a]                         (as pfv_transport_advance_multi)
 * with A = div diag(q) U of the one-component discretization on the handle (pfv_upwind_discretize with
 * num_components = 1; no pfv_upwind_assemble is needed).  rate = K (k x k, row-major, host memory) is the rate matrix of
 * dc/dt = -K c, shared by all cells; rate_weight = rho (Nc, NULL = 1, >= 0) the weight of the reaction term per cell
 * (pore volume x dt, a reactive zone, a temperature factor); mobility = w (k, host memory, NULL = 1, >= 0): w_a = 0 is an
 * immobile component (a sorbed phase, matrix porosity, biomass) that sees no flux and no boundary -- its bc_values[a] are
 * not read --, w_a = 1 what pfv_transport_advance_multi does.
 *   Admissible K, else PFV_ERR_ARGUMENT: K_aa >= 0; K_ab <= 0 for a != b; every column sum
 * sum_a K_ab >= -k 2^-52 sum_a |K_ab| (no mass created, up to the rounding of a sum of k terms).  With accumulation > 0
 * every row block B_i = diag(acc_ia + w_a A_ii) + rho_i K then is a strictly column-diagonally-dominant M-matrix: it is
 * eliminated WITHOUT pivoting, non-negative data give non-negative concentrations, and block Jacobi converges on a
 * cyclic core.  Decay chains, A <-> B, mobile <-> immobile pairs and yields <= 1 are covered; there is no pivoted path.
 *   In flow order a cell is one k x k solve in registers once its upstream cells are known (csrc/sweep.inc:
 * sweep_row_react<k>), in the launches of one component: pfv_stats.sweep_launches is that of pfv_transport_advance
 * with PFV_PRECOND_SWEEP on the same flux.  The cells of a cyclic core are iterated by block Jacobi until every component
 * has ||F_core,a|| <= rtol ||g_a|| / 2, or maxit iterations.  A step is accepted when every component has
 * ||F_a|| <= rtol ||g_a|| (0 <= 0 counts) with F_a the residual of its equations and the scale
 * g_a = rhs_a - rho sum_{b != a} K_ab c_b, rhs_a = acc_a o c_old_a - w_a b_ref_a + src_a: a daughter that starts from
 * nothing has rhs_a = 0 and lives on what its parent produces.  One host read per step brings the 2 k norms.
 *   bc_values [k][Nf], accumulation, source (may be NULL) and c (in and out) [k][Nc] are component-major and follow
 * pfv_set_vectors_on_device, as rate_weight and q (Nf, NULL = the flux of the discretization) do; on the device the
 * vectors are cell-major and interleaved, v[i * k + a].  c holds the state after the last accepted step; a refused
 * step returns the state of that step's start, steps_done and PFV_ERR_NOT_CONVERGED.  last (k entries, may be NULL):
 * iterations = 1 for an acyclic flux, else the core iterations of the last step; rel_residual the measured
 * ||F_a|| / ||g_a||.
 *   PFV_ERR_ARGUMENT (the text names the first offender, the lowest cell or face and its lowest component): no
 * discretization or num_components != 1; k outside 1 .. 8; a K that breaks the conditions above or is not finite; a
 * negative or non-finite mobility; a negative or NaN rate_weight; accumulation <= 0 or NaN; a non-finite c; a
 * non-finite bc_values[a] on a Dirichlet inflow or Neumann face of a component with w_a > 0; a boundary face with inflow
 * that is neither Dirichlet nor Neumann.  PFV_ERR_UNSUPPORTED: periodic grids, conditions per sub-face, the sharded
 * solve, (k + 1) max(Nc, Nf) >= 2^31.  The handle rules are those of pfv_transport_advance_nl: the flow order is built
 * if the handle has none for this flux, whatever preconditioner is selected; the selection and the flow system are left
 * alone; no transport system is left behind.  pfv_stats: transport_react_* and the sweep_* fields. */
pfv_status pfv_transport_advance_react(pfv_ctx* h, const double* q, int k, const double* bc_values,
                                       const double* accumulation, const double* source, const double* mobility,
                                       const double* rate, const double* rate_weight, int n_steps, double rtol,
                                       int maxit, double* c, int32_t* steps_done, pfv_solve_info* last);

/* Sorbing transport: n_steps implicit Euler steps of k (1 .. 64) concentrations c >= 0 in equilibrium with a sorbed
 * amount on a NONLINEAR isotherm, on the flux q -- Freundlich or Langmuir retardation.  Per cell i and component a
 *     acc_ia (c_ia - c_old_ia) + cap_ia (S_a(c_ia) - S_a(c_old_ia)) + sum_j A_ij c_ja + b_ref_ia = src_ia
 *     b_ref_a = div (rhs_neu + rhs_dir diag(q)) bc_values[a]                         (as pfv_transport_advance_multi)
 * with A = div diag(q) U of the one-component discretization on the handle (pfv_upwind_discretize with
 * num_components = 1; no pfv_upwind_assemble is needed).  accumulation = acc > 0 is porosity x volume / dt; capacity =
 * cap >= 0 ([k][Nc], NULL: no sorption) is bulk density x volume / dt and carries whatever scales the isotherm per cell.
 * isotherm_kind (k values, host memory) names a PFV_ISOTHERM_* per component, isotherm_params ([k][2], host memory) its
 * two parameters.  The call is for c >= 0; pfv_transport_advance_multi remains the call for signed quantities.
 *   In flow order the step is one scalar monotone root-finding per cell and component (csrc/sweep.inc: sweep_row_sorb):
 * with d = A_ii and R = rhs - sum_upstream A_ij c_j the unknown solves g(x) = (acc + d) x + cap S(x) - R = 0 on the
 * bracket [0, R / (acc + d)], by Newton from the state of the step's start, safeguarded by bisection; the transport
 * part stays linear, so there is no Jacobian, no Krylov loop and no damping, and an acyclic flux is solved exactly.  A
 * linear component is folded into the accumulation, acc + cap Kd, and is the division of pfv_transport_advance_multi:
 * with Kd = 1 its bits are those of that call with accumulation = acc + cap and PFV_PRECOND_SWEEP on an acyclic flux.
 * S(c) of a row is carried beside c for the next step's right-hand side rhs = acc c_old + cap S(c_old) - b_ref + src: no
 * power is evaluated outside the root-finder.  All k components go in the launches of one: pfv_stats.sweep_launches
 * is that of pfv_transport_advance with PFV_PRECOND_SWEEP on the same flux, and a component's result on an acyclic flux
 * does not depend on which other components ride in the call.  The cells of a cyclic core are iterated by nonlinear
 * Jacobi until every component has ||F_core,a|| <= rtol ||rhs_a|| / 2, or maxit iterations.  A step is accepted when
 * every component has ||F_a|| <= rtol ||rhs_a|| (0 <= 0 counts), F_a = rhs_a - (acc c + cap S(c) + A c); one host read
 * per step brings the 2 k norms and the flag word.  There is no per-component fallback.
 *   bc_values [k][Nf], accumulation, capacity (may be NULL), source (may be NULL), c (in and out) and sorbed_out (may be
 * NULL: S_a(c_a) of the returned state) [k][Nc] are component-major and follow pfv_set_vectors_on_device, as q (Nf,
 * NULL = the flux of the discretization) does.  c holds the state after the last accepted step.  last (k entries, may
 * be NULL): iterations = 1 for an acyclic flux, else the core iterations of the last step; rel_residual the measured
 * ||F_a|| / ||rhs_a||.
 *   A row with R < 0 beyond rounding has no root c >= 0 (a sink that takes more than the cell holds): the step is refused
 * with PFV_ERR_ARGUMENT and the text "step N leaves c >= 0: no root in cell I, component A" (the lowest such cell, its
 * lowest component); c is the state before that step.  PFV_ERR_ARGUMENT too, the text naming the lowest offender: no
 * discretization or num_components != 1; k outside 1 .. 64; an unknown isotherm kind, a non-finite parameter, a
 * negative Kd, Kf, q_max or b, n <= 0; accumulation <= 0 or NaN; a negative or NaN capacity; a c that is negative or
 * not finite; a negative or non-finite bc_values[a] on a Dirichlet inflow face, a non-finite one on a Neumann face; a
 * boundary face with inflow that is neither Dirichlet nor Neumann.  PFV_ERR_NOT_CONVERGED: a core that did not settle,
 * a step whose check fails; c is the state of that step's start.  PFV_ERR_UNSUPPORTED and the handle rules are those
 * of pfv_transport_advance_react: the flow order is built if the handle has none for this flux and stays; the
 * preconditioner selection and the flow system are left alone; no transport system is left behind.  pfv_stats:
 * transport_sorb_* and the sweep_* fields. */
pfv_status pfv_transport_advance_sorb(pfv_ctx* h, const double* q, int k, const int32_t* isotherm_kind,
                                      const double* isotherm_params, const double* bc_values,
                                      const double* accumulation, const double* capacity, const double* source,
                                      int n_steps, double rtol, int maxit, double* c, double* sorbed_out,
                                      int32_t* steps_done, pfv_solve_info* last);

/* The adjoint of pfv_transport_advance_multi: every gradient of J = sum_{n=1..N} sum_a <g_a^n, c_a^n> through n_steps = N
 * forward steps (diag(acc_a) + A(q)) c_a^n = acc_a o c_a^{n-1} - b_ref(q, bv_a) + src_a, for the cost of about one more
 * run.  For n = N .. 1 the call solves S_a^T lambda_a^n = g_a^n + acc_a o lambda_a^{n+1} (lambda^{N+1} = 0) for all
 * n_comp components by ONE transposed substitution in reverse flow order (csrc/sweep.inc: sweep_row_multi_t): the
 * levels, the launch plan and the load chain per row are those of the forward sweep.  The cells of a cyclic core are
 * iterated by Jacobi on their transposed rows until ||residual_core,a|| <= rtol ||rhs_a|| / 2 for every component, or
 * maxit iterations.  A step is accepted when ||rhs_a - S_a^T lambda_a|| <= rtol ||rhs_a|| holds for every component
 * (0 <= 0 counts); one host read per step brings the 2 n_comp norms.  There is no per-component fallback.
 *   loads [N][n_comp][n_obs]: loads[n - 1] = g^n = dJ/dc^n on the observation cells obs_cells (n_obs int32 cell indices
 * in HOST memory, no repeats; NULL: every cell in order, n_obs must be Nc).  states (may be NULL): c^0 .. c^N as
 * [N + 1][n_comp][Nc]; one slab is staged per step.  q (Nf, NULL = the flux of the discretization), bc_values
 * [n_comp][Nf], accumulation [n_comp][Nc], loads and states follow pfv_set_vectors_on_device, as the gradients do.
 *   Gradients, each may be NULL (not wanted), all accumulated on the device without floating-point atomics:
 *     grad_c0 [n_comp][Nc]           acc_a o lambda_a^1
 *     grad_source [n_comp][Nc]       sum_n lambda_a^n
 *     grad_bc_values [n_comp][Nf]    -sum_n B^T lambda_a^n, B = div (rhs_neu + rhs_dir diag(q)): non-zero on Neumann faces
 *                                    and on Dirichlet inflow faces only
 *     grad_accumulation [n_comp][Nc] sum_n lambda_a^n o (c_a^{n-1} - c_a^n)                          (needs states)
 *     grad_flux [Nf]                 -sum_n sum_a (lambda_a^n[p] - lambda_a^n[m]) cup_a^n[f]         (needs states)
 * with p / m the cells of cell_faces sign +1 / -1 at f (a missing cell contributes nothing) and cup the value the upwind
 * rule takes at f: the upstream cell's c^n on interior and outflow faces, bc_values on a Dirichlet inflow face; 0 on a
 * Neumann face, whose flux is data.  grad_flux is the derivative at a FIXED upstream side: it is the derivative of J
 * wherever no q_f is exactly zero, and a one-sided one there.
 *   Requirements as pfv_transport_advance_multi: a one-component discretization on the handle, n_comp in 1 .. 64,
 * n_comp x Nc and n_comp x Nf below 2^31 (PFV_ERR_UNSUPPORTED); a zero or NaN diagonal A[i,i] + accumulation[a][i] is
 * PFV_ERR_UNSUPPORTED naming the row and the component.  PFV_ERR_ARGUMENT (the text names the offender): an obs_cells
 * entry out of range or repeated; grad_accumulation or grad_flux without states; a non-finite value in loads.
 *   steps_done: the adjoint steps completed.  A refused step returns PFV_ERR_NOT_CONVERGED and writes no gradient.
 * last (n_comp entries, may be NULL): iterations = 1 for an acyclic flux, else the core iterations of the last step;
 * rel_residual the measured ||rhs_a - S_a^T lambda_a|| / ||rhs_a||.  The flow order is built if the handle has none
 * for this flux, whatever preconditioner is selected, and stays; the selection and the flow system are left alone; no
 * transport system is left behind (pfv_solve asks for an assembly).  pfv_stats: transport_adjoint_* and the sweep_*
 * fields (sweep_launches: those of one transposed sweep -- the forward sweep's on an acyclic flux). */
pfv_status pfv_transport_adjoint_multi(pfv_ctx* h, const double* q, int n_comp, const double* bc_values,
                                       const double* accumulation, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                       const double* loads, const double* states, double rtol, int maxit,
                                       double* grad_c0, double* grad_source, double* grad_bc_values,
                                       double* grad_accumulation, double* grad_flux, int32_t* steps_done,
                                       pfv_solve_info* last);

/* The adjoint of pfv_transport_advance_react: every gradient of J = sum_{n=1..N} sum_a <g_a^n, c_a^n> through n_steps = N
 * forward steps acc_a o (c_a^n - c_a^{n-1}) + w_a (A(q) c_a^n + b_ref_a) + rho o sum_b K_ab c_b^n = src_a.  The step is
 * linear in c, so the adjoint is exact: for n = N .. 1 all k components solve ONE system
 * M^T lambda^n = g^n + acc o lambda^{n+1} (lambda^{N+1} = 0).  In reverse flow order cell i is one k x k solve
 *     B_i^T lambda_i = R_i,  B_i = diag(acc_ia + w_a A_ii) + rho_i K,  R_ia = r_ia - w_a sum_{lev[j] > lev[i]} valT[e] lambda_ja
 * (csrc/sweep.inc: sweep_row_react<k, Descending>, the forward row with the transposed values and K^T): the levels and
 * the launch plan are those of the forward sweep.  B_i^T is a strictly row-diagonally-dominant M-matrix; it is
 * eliminated WITHOUT pivoting (growth factor <= 2), there is no pivoted path.  The cells of a cyclic core are iterated
 * by block Jacobi from zero until every component has ||F_core,a|| <= rtol ||g~_a|| / 2, or maxit iterations.  A step is
 * accepted when every component has ||F_a|| <= rtol ||g~_a|| (0 <= 0 counts), F_a = r_a - (M^T lambda)_a and the scale
 * g~_a = r_a - rho sum_{b != a} K_ba lambda_b (a parent that is observed only through its daughter has r_a = 0).  One host
 * read per step brings the 2 k norms and the status word.
 *   k, bc_values, accumulation, mobility, rate, rate_weight and q are those of pfv_transport_advance_react, with its
 * rules and texts (rate is checked as the caller passes it, not its transpose; bc_values[a] of an immobile component
 * is not read and may be NaN); loads, obs_cells, states and the first five gradients are those of
 * pfv_transport_adjoint_multi.  rate and mobility are HOST memory, and so is grad_rate (k^2 doubles); every other
 * array follows pfv_set_vectors_on_device.  states are NOT checked for finiteness.
 *   Gradients, each may be NULL (not wanted), all accumulated on the device without floating-point atomics:
 *     grad_c0 [k][Nc]            acc_a o lambda_a^1
 *     grad_source [k][Nc]        sum_n lambda_a^n
 *     grad_bc_values [k][Nf]     -w_a sum_n B^T lambda_a^n; all zero for w_a = 0
 *     grad_accumulation [k][Nc]  sum_n lambda_a^n o (c_a^{n-1} - c_a^n)                               (needs states)
 *     grad_flux [Nf]             -sum_n sum_a w_a (lambda_a^n[p] - lambda_a^n[m]) cup_a^n[f], at a fixed upstream side;
 *                                components with w_a = 0 are skipped                                   (needs states)
 *     grad_rate [k][k]           -sum_n sum_i rho_i lambda_ia^n c_ib^n: the plain partial derivative with respect to
 *                                EVERY entry of K, structural zeros included; the chain to the caller's rate
 *                                parameters is the caller's                                            (needs states)
 *     grad_rate_weight [Nc]      -sum_n sum_a lambda_ia^n sum_b K_ab c_ib^n                            (needs states)
 * The k^2 sums of grad_rate run over a fixed partition of the cells that depends on Nc and k alone and are added in
 * step order: the result does not depend on the launch form of the sweep or on a repeat of the call.  The gradient
 * with respect to the mobility is not offered (it needs the boundary values of immobile components).
 *   PFV_ERR_ARGUMENT (the text names the offender): what pfv_transport_advance_react refuses in its arguments; an
 * obs_cells entry out of range or repeated; a non-finite value in loads; grad_accumulation, grad_flux, grad_rate or
 * grad_rate_weight without states.  PFV_ERR_UNSUPPORTED as pfv_transport_advance_react.
 *   steps_done: the adjoint steps completed.  A refused step returns PFV_ERR_NOT_CONVERGED and writes no gradient.
 * last (k entries, may be NULL): iterations = 1 for an acyclic flux, else the core iterations of the last step;
 * rel_residual the measured ||F_a|| / ||g~_a||.  Handle rules as pfv_transport_adjoint_multi: the flow order is built
 * if needed and stays, the transposed positions stay with the pattern, the selection and the flow system are left
 * alone, no transport system is left behind.  pfv_stats: transport_react_adjoint_* and the sweep_* fields
 * (sweep_launches: the forward sweep's on an acyclic flux). */
pfv_status pfv_transport_adjoint_react(pfv_ctx* h, const double* q, int k, const double* bc_values,
                                       const double* accumulation, const double* mobility, const double* rate,
                                       const double* rate_weight, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                       const double* loads, const double* states, double rtol, int maxit,
                                       double* grad_c0, double* grad_source, double* grad_bc_values,
                                       double* grad_accumulation, double* grad_flux, double* grad_rate,
                                       double* grad_rate_weight, int32_t* steps_done, pfv_solve_info* last);

/* The adjoint of pfv_transport_advance_nl: every gradient of J = sum_{n=1..N} <g^n, s^n[obs_cells]> through n_steps = N
 * saturation steps acc o (s^n - s^{n-1}) + M f(s^n) + b_ref(q, f(bv)) = source, M = A(q) + diag(sink).  The step is
 * linearised about the forward states: with d^n = f'(s^n) (one-sided, as the step's own Newton uses it) and
 * lambda^{N+1} = 0 the call solves, for n = N .. 1,
 *     (diag(acc) + diag(d^n) M^T) lambda^n = g^n + acc o lambda^{n+1}.
 * In reverse flow order cell i is one division once the cells downstream of it are known (csrc/sweep.inc: sweep_row_nl_t),
 *     lambda_i = (r_i - d_i sum_{lev[j] > lev[i]} valT[e] lambda_j) / (acc_i + d_i (A_ii + sink_i)):
 * the levels, the launch plan and the launch count are those of the forward sweep, and there is no root-finding.  d^n
 * and f(s^n) come from one streaming pass over the step's slab of states.  The Jacobian is strictly column-diagonally
 * dominant (acc > 0), so the cells of a cyclic core converge under Jacobi on their transposed rows, from zero, until
 * ||residual_core|| <= rtol ||rhs|| / 2 or maxit iterations.  A step is accepted when ||r - J^T lambda|| <= rtol ||r||
 * (0 <= 0 counts); one host read per step.  A cell at or beyond a residual saturation (d_i = 0) is acc_i lambda_i = r_i.
 *   fluxfn_kind / fluxfn_params / n_params, q, bc_values, accumulation and sink are those of pfv_transport_advance_nl,
 * with its rules and texts (the source does not enter).  loads [N][n_obs] and obs_cells are those of
 * pfv_transport_adjoint_multi with one component.  states [N + 1][Nc], s^0 .. s^N, is REQUIRED (PFV_ERR_ARGUMENT when
 * NULL with n_steps > 0); one slab is staged per step; it is NOT checked for range or finiteness.  fluxfn_params and
 * grad_fluxfn are HOST memory; every other array follows pfv_set_vectors_on_device.
 *   Gradients, each may be NULL (not wanted), all accumulated on the device without floating-point atomics, every sum
 * in a fixed order; p / m are the cells of cell_faces sign +1 / -1 at a face (a missing cell contributes nothing):
 *     grad_s0 [Nc]            acc o lambda^1
 *     grad_source [Nc]        sum_n lambda^n
 *     grad_bc_values [Nf]     Neumann face: -sum_n (rhs_neu^T div^T lambda^n)_f; Dirichlet inflow face:
 *                             -sum_n (lambda^n[p] - lambda^n[m]) q_f f'(bv_f); 0 on every other face
 *     grad_accumulation [Nc]  sum_n lambda^n o (s^{n-1} - s^n)
 *     grad_sink [Nc]          -sum_n lambda^n o f(s^n); with sink == NULL the derivative at sink = 0
 *     grad_flux [Nf]          -sum_n (lambda^n[p] - lambda^n[m]) phiup_f^n, phiup = f of the upstream cell's s^n on interior
 *                             and outflow faces, f(bv_f) on a Dirichlet inflow face, 0 on a Neumann face
 *     grad_fluxfn [6]         PFV_FLUXFN_COREY only (else PFV_ERR_ARGUMENT), in the order of its parameters:
 *                             -sum_n [ sum_i (M^T lambda^n)_i df/dtheta(s_i^n)
 *                                      + sum_{Dirichlet inflow f} (lambda^n[p] - lambda^n[m]) q_f df/dtheta(bv_f) ],
 *                             df/dtheta analytic (csrc/fluxfn.h: fluxfn_eval_params), 0 where s_e lies outside (0, 1)
 * All are derivatives on a FIXED branch: of the table's interval, of the side of a residual saturation, of the upstream
 * side of every face.  They are the derivatives of J wherever no state sits on a table knot or a residual saturation
 * and no q_f is exactly zero, and one-sided ones there.  The six sums of grad_fluxfn run over a fixed partition that
 * depends on Nc and Nf alone and are added in step order: the result does not depend on the launch form or a repeat.
 *   PFV_ERR_ARGUMENT (the text names the offender): what pfv_transport_advance_nl refuses in the flux function,
 * accumulation, sink, bc_values and the inflow faces; an obs_cells entry out of range or repeated; a non-finite value
 * in loads; missing states; grad_fluxfn with another kind.  PFV_ERR_UNSUPPORTED as pfv_transport_advance_nl.
 *   steps_done: the adjoint steps completed.  A refused step returns PFV_ERR_NOT_CONVERGED and writes no gradient.
 * last (one entry, may be NULL): iterations = 1 for an acyclic flux, else the core iterations of the last step;
 * rel_residual the measured ||r - J^T lambda|| / ||r||.  Handle rules as pfv_transport_adjoint_multi: the flow order is
 * built if needed and stays, the transposed positions stay with the pattern, the selection and the flow system are left
 * alone, no transport system is left behind.  pfv_stats: transport_nl_adjoint_* and the sweep_* fields (sweep_launches:
 * the forward sweep's on an acyclic flux). */
pfv_status pfv_transport_adjoint_nl(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                    int n_params, const double* bc_values, const double* accumulation,
                                    const double* sink, int n_steps, int64_t n_obs, const int32_t* obs_cells,
                                    const double* loads, const double* states, double rtol, int maxit, double* grad_s0,
                                    double* grad_source, double* grad_bc_values, double* grad_accumulation,
                                    double* grad_sink, double* grad_flux, double* grad_fluxfn, int32_t* steps_done,
                                    pfv_solve_info* last);

/* The adjoint of pfv_transport_advance_nl_multi: the gradients of
 *     J = sum_{n=1..N} [ <s_loads[n-1], s^n[obs_cells]> + sum_a <c_loads[n-1][a], c_a^n[obs_cells]> ]
 * through n_steps = N steps of the saturation with k phase-carried components -- what a match of tracer, salinity or
 * polymer breakthrough curves by Corey parameters, porosity, well rates or the flux needs.  With lambda the multiplier
 * of the saturation's equation and mu_a that of component a's, M = A + diag(sink), phi^n = f(s^n), d^n = f'(s^n),
 * e_a^n = acc o s^n + sorption_a and lambda^{N+1} = mu_a^{N+1} = 0 the call solves, for n = N .. 1,
 *     (diag(e_a^n) + diag(phi^n) M^T) mu_a^n = c_loads_a^n + e_a^n o mu_a^{n+1}
 *     (diag(acc) + diag(d^n) M^T) lambda^n  = s_loads^n + acc o lambda^{n+1}
 *                                              - sum_a c_a^n o [acc o (mu_a^n - mu_a^{n+1}) + d^n o (M^T mu_a^n)].
 * In reverse flow order cell i is k + 1 divisions once the cells downstream of it are known (csrc/sweep.inc:
 * sweep_row_nlc_t): with o = A_ii + sink_i and u_a = sum_{lev[j] > lev[i]} valT[e] mu_aj,
 *     mu_ai = (rmu_ai - phi_i u_a) / (acc_i s_i + sorption_ai + phi_i o),   (M^T mu_a)_i = u_a + o mu_ai,
 * so the coupling term is known inside the row and lambda_i is the division of pfv_transport_adjoint_nl on the reduced
 * right-hand side: ONE fused transposed sweep per step, with the levels, the launch plan and the launch count of the
 * forward sweep.  The cells of a cyclic core iterate mu and lambda jointly by Jacobi on their transposed rows (the
 * system is block triangular: the rate is that of its diagonal blocks), from zero, until every one of the k + 1
 * residuals of the core is below rtol / 2 of its scale, at most maxit times.  A step is accepted when all k + 1
 * residuals pass ||r - image|| <= rtol ||r|| (0 <= 0 counts); lambda's right-hand side in that check is recomputed from
 * the image of the final mu.  One host read per step.
 *   fluxfn_kind / fluxfn_params / n_params, q, bc_values, accumulation, sink, k, c_bc_values [k][Nf] and sorption
 * [k][Nc] (may be NULL) are those of pfv_transport_advance_nl_multi, with its rules and texts (the sources do not
 * enter).  s_loads [N][n_obs] and c_loads [N][k][n_obs] with obs_cells as in pfv_transport_adjoint_multi; either may be
 * NULL (zeros), not both.  s_states [N + 1][Nc] and c_states [N + 1][k][Nc] are REQUIRED (PFV_ERR_ARGUMENT when NULL
 * with n_steps > 0); one slab of each is staged per step; they are NOT checked for range or finiteness.  fluxfn_params
 * and grad_fluxfn are HOST memory; every other array follows pfv_set_vectors_on_device.
 *   Gradients, each may be NULL (not wanted), accumulated on the device in step order without floating-point atomics;
 * p / m are the cells of cell_faces sign +1 / -1 at a face (a missing cell contributes nothing):
 *     grad_s0 [Nc]              acc o lambda^1 + sum_a acc o c_a^0 o mu_a^1
 *     grad_c0 [k][Nc]           (acc o s^0 + sorption_a) o mu_a^1
 *     grad_source [Nc]          sum_n lambda^n
 *     grad_c_source [k][Nc]     sum_n mu_a^n
 *     grad_accumulation [Nc]    -sum_n [lambda^n o (s^n - s^{n-1}) + sum_a mu_a^n o (s^n o c_a^n - s^{n-1} o c_a^{n-1})]
 *     grad_sorption [k][Nc]     -sum_n mu_a^n o (c_a^n - c_a^{n-1}); with sorption == NULL the derivative at zero
 *     grad_sink [Nc]            -sum_n phi^n o (lambda^n + sum_a mu_a^n o c_a^n)
 *     grad_bc_values [Nf]       the saturation's boundary value.  Neumann face: as pfv_transport_adjoint_nl, from lambda
 *                               alone.  Dirichlet inflow face: -sum_n q_f f'(bv_f) [(lambda[p] - lambda[m]) +
 *                               sum_a (mu_a[p] - mu_a[m]) cbv_af]
 *     grad_c_bc_values [k][Nf]  Neumann face: -sum_n (rhs_neu^T div^T mu_a^n)_f.  Dirichlet inflow face:
 *                               -sum_n (mu_a[p] - mu_a[m]) q_f f(bv_f).  0 on every other face
 *     grad_flux [Nf]            -sum_n [(lambda[p] - lambda[m]) phiup_f + sum_a (mu_a[p] - mu_a[m]) phiup_f cup_af]: phiup as
 *                               in pfv_transport_adjoint_nl, cup the upstream cell's c_a^n (interior and outflow faces),
 *                               cbv_af on a Dirichlet inflow face; 0 on a Neumann face
 *     grad_fluxfn [6]           PFV_FLUXFN_COREY only (else PFV_ERR_ARGUMENT): the sums of pfv_transport_adjoint_nl with the
 *                               cell weight (M^T lambda)_i + sum_a c_ai (M^T mu_a)_i and the face weight
 *                               q_f [(lambda[p] - lambda[m]) + sum_a (mu_a[p] - mu_a[m]) cbv_af]
 * All are derivatives on a FIXED branch, as those of pfv_transport_adjoint_nl.
 *   A dry row -- acc_i s_i^n + sorption_ai + phi_i o_i = 0, where the forward step keeps c and does not determine it -- is
 * refused with PFV_ERR_ARGUMENT naming the step, the cell and the component (found in the streaming pass over the slab,
 * read with the step's norms).  Rows with d_i = 0 are legal.  PFV_ERR_ARGUMENT otherwise as pfv_transport_advance_nl_multi
 * and pfv_transport_adjoint_nl; PFV_ERR_UNSUPPORTED as pfv_transport_advance_nl_multi.
 *   steps_done: the adjoint steps completed.  A refused step returns PFV_ERR_NOT_CONVERGED and writes no gradient.
 * last (1 + k entries, may be NULL): the saturation's, then the components'; iterations = 1 for an acyclic flux, else
 * the core iterations of the last step; rel_residual the measured ones.  Handle rules as pfv_transport_adjoint_nl.
 * pfv_stats: transport_nlc_adjoint_* and the sweep_* fields (sweep_launches: the forward sweep's on an acyclic flux). */
pfv_status pfv_transport_adjoint_nl_multi(pfv_ctx* h, const double* q, int fluxfn_kind, const double* fluxfn_params,
                                          int n_params, const double* bc_values, const double* accumulation,
                                          const double* sink, int k, const double* c_bc_values, const double* sorption,
                                          int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* s_loads,
                                          const double* c_loads, const double* s_states, const double* c_states,
                                          double rtol, int maxit, double* grad_s0, double* grad_c0, double* grad_source,
                                          double* grad_c_source, double* grad_accumulation, double* grad_sorption,
                                          double* grad_sink, double* grad_bc_values, double* grad_c_bc_values,
                                          double* grad_flux, double* grad_fluxfn, int32_t* steps_done,
                                          pfv_solve_info* last);

/* ---- Adjoint of the flow solve (csrc/flow_adjoint.inc): where the grad_flux of the transport adjoints goes on ------
 * The linear flow problem of the discretization on the handle, div = cell_faces^T:
 *     q = T p + B bc (+ V g),      A p = source - div (B bc + V g),      A = div T
 * (T, B, V = PFV_MAT_FLUX, PFV_MAT_BOUND_FLUX, PFV_MAT_VECTOR_SOURCE).  For an objective J with g_q = dJ/dq = load_flux
 * (Nf) and g_p = dJ/dp = load_pressure (Nc) at the forward solution -- at least one of the two, else PFV_ERR_ARGUMENT --
 *     A^T mu = g_p + T^T g_q                       one transposed solve
 *     z_f    = g_q[f] - sum_{e of f} sgn_e mu_c(e)
 *     grad_source [Nc]          mu
 *     grad_bc_values [Nf]       B^T z                                           (zero off the boundary)
 *     grad_perm [(3,3,Nc)]      sum_{e=(c,f)} z_f w_f t_f^2 sgn_e d_r n_s / (t_e^2 |d|^2), layout of perm_33n, all nine
 *                               entries independent (the derivative of pfv_tpfa_transmissibility_ad)
 * w_f = d q_f / d t_f = filter_f (p_diff_f + g_diff_f) - dir_f sgn_f bc_f as pfv_mpfa_ad_flux_system defines it (filter 0
 * on Neumann faces).  What grad_perm means depends on the discretization.  pfv_tpfa_discretize: the exact gradient of
 * the discrete problem.  pfv_mpfa_discretize: grad_source, grad_bc_values and mu are exact; grad_perm is the two-point
 * product rule of the reference's AdTpfaFlux -- the same approximation pfv_mpfa_ad_flux_system makes for its Jacobian
 * --, NOT the derivative of the MPFA matrices: that derivative is the grad_perm_exact of pfv_flow_adjoint_exact below
 * (on a K-orthogonal grid the two agree; on tetrahedra with a full tensor they do not, and the entries K_rs, r != s,
 * have no meaningful two-point derivative).  The gradient with respect to the vector source is not formed.
 *   p (Nc) is the forward solution: the caller's responsibility, not checked against the system.  bc_values (Nf) and
 * vector_source (per cell as pfv_mpfa_assemble takes it, or NULL) as in the forward solve.  mu_out (Nc), grad_perm,
 * grad_bc_values and grad_source may each be NULL.  All vectors follow pfv_set_vectors_on_device: a grad_flux left in
 * device memory by a transport adjoint is consumed without a host visit.
 *   The solve: A = div T is assembled afresh (an earlier pfv_mpfa_ad_flux_system may have left J in its value array), its
 * transposed values are taken on its own pattern through transposed positions (the pattern of div T is structurally
 * symmetric; a missing partner is PFV_ERR_UNSUPPORTED), and (A^T, g_p + T^T g_q) becomes the active system of one
 * pfv_solve with the preconditioner selected on the handle; method, rtol, maxit, restart as in pfv_solve, info receives
 * its info.  A solve that does not converge returns PFV_ERR_NOT_CONVERGED and writes no output.  T^T and B^T are
 * gathers over column maps of the two patterns (entries sorted by (column, row)), built on first use and kept with
 * the patterns; no floating-point atomics, two calls give the same bits.
 *   After the call the handle holds NO active system (pfv_solve asks for an assembly, as after the transport calls);
 * the discretization, the resident face flux, the upwind discretization and the flow order are untouched.
 *   PFV_ERR_ARGUMENT: no flow discretization with per-face conditions on the handle; no load; a non-finite value in a
 * load, in p or in bc_values on a boundary face (the text names the lowest index).  PFV_ERR_UNSUPPORTED (the text names
 * the first offending face where there is one): Robin faces, faces flagged PFV_BC_INTERNAL, periodic grids, conditions
 * per sub-face, partial discretizations with zeroed rows, the sharded solve, a flux pattern of 2^31 entries or more.
 * pfv_stats: flow_adjoint_*. */
pfv_status pfv_flow_adjoint(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                            const double* load_flux, const double* load_pressure, int method, double rtol, int maxit,
                            int restart, double* mu_out, double* grad_perm, double* grad_bc_values,
                            double* grad_source, pfv_solve_info* info);

/* The same call -- the same checks and refusals, the same solve, the same bits in every output of pfv_flow_adjoint --
 * with one more output from the same mu (csrc/mpfa_adjoint.inc):
 *     grad_perm_exact [(3,3,Nc)]   d/dK of z^T (T p + B bc + V g) at fixed p, bc, g: the exact gradient of J with respect
 *                                  to the permeability of the discrete problem, layout of perm_33n, all nine entries
 *                                  independent (on a 2-D grid only the 2 x 2 block is non-zero); NULL: not formed.
 * pfv_mpfa_discretize: K enters the interaction region of a node only through nK_h = n_h^T K_c.  One pass over the
 * regions (one per wavefront, the condensed system of the discretization set up afresh in LDS, ONE pivoted inverse)
 * solves the region for the actual p, bc and g (u_j = g_j - gamma_j per sub-cell), solves its transposed system for the
 * load -z_f(s) omega_{h*(s)} of the sub-face fluxes (nu), and leaves per sub-half-face h = (j, l) of cell c
 *     ( -z_f(s) [h = h*(s)] - nu_l sgn_h [row l not Dirichlet] ) n_h[r] u_j[b]        in grad[r][b][c];
 * the sub-cells of a cell are summed by a second kernel in the fixed order of a cell -> sub-cell map kept with the
 * sub-cell topology (no floating-point atomics; two calls give the same bits).  The table rows and sub-face records of
 * the discretization are not touched.  pfv_tpfa_discretize: grad_perm_exact = grad_perm.
 *   Further statuses: PFV_ERR_UNSUPPORTED names the node whose interaction region does not fit the LDS (found before the solve);
 * PFV_ERR_SINGULAR names the node as pfv_mpfa_discretize does.  A refused call writes no output.
 * pfv_stats: flow_adjoint_exact_*. */
pfv_status pfv_flow_adjoint_exact(pfv_ctx* h, const double* p, const double* bc_values, const double* vector_source,
                                  const double* load_flux, const double* load_pressure, int method, double rtol,
                                  int maxit, int restart, double* mu_out, double* grad_perm, double* grad_perm_exact,
                                  double* grad_bc_values, double* grad_source, pfv_solve_info* info);

/* ---- Advection-diffusion step on the device (csrc/advdiff.inc) ---------------------------------------------------
 * One handle carries the transport keyword: its diffusion discretization (pfv_mpfa_discretize or pfv_tpfa_discretize
 * of the keyword's tensor and conditions) and the upwind classification of its faces, decided from sign(q) with the
 * same flags (pfv_mpfa_set_params) by the rules of pfv_upwind_discretize.  The system
 *     S = diag(accumulation) + div flux_D + w div diag(q) U            (PFV_MAT_ADVDIFF_SYSTEM, pattern of PFV_MAT_SYSTEM)
 *     r = accumulation o c_old - b_ref + b_D + source
 * with b_D = -div bound_flux_D bc_values and b_ref = div (rhs_neu + rhs_dir diag(w q)) bc_values becomes the active
 * system of pfv_solve.  div flux_D and b_D are formed once per discretization and kept; every later call refreshes the
 * values of S, its diagonal and r in one kernel, without symbolic work and without pfv_upwind_discretize.
 * q (Nf): NULL = the resident face flux of this handle; with vectors on the device it may be the resident flux of
 * another handle on the same device (pfv_resident_flux).  flux_scale w must be positive and finite.  bc_values (Nf):
 * NULL = those of the previous call on this discretization.  accumulation, c_old, source (Nc) and bound_rhs_out (Nc,
 * receives b_ref) may be NULL.  A boundary face with inflow that is neither Dirichlet nor Neumann: PFV_ERR_ARGUMENT.
 * Periodic grids, conditions per sub-face, Robin faces and the sharded solve: PFV_ERR_UNSUPPORTED.  The solver caches
 * are invalidated as by pfv_upwind_assemble; the AMG aggregate maps are kept, so the next setup reuses them. */
pfv_status pfv_advdiff_assemble(pfv_ctx* h, const double* q, double flux_scale, const double* bc_values,
                                const double* accumulation, const double* c_old, const double* source,
                                double* bound_rhs_out);
/* n_steps implicit Euler steps with the system of pfv_advdiff_assemble, the state resident between the steps: per step
 * r = accumulation o c - b_ref + b_D + source, then a solve with the preconditioner selected on the handle
 * (pfv_set_preconditioner: PFV_PRECOND_JACOBI, PFV_PRECOND_AMG -- the hierarchy is set up once and reused by all steps --
 * or PFV_PRECOND_SWEEP, the flow order built once and, like AMG, backed by the Jacobi-GMRES fallback below)
 * started from c.  method: PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES.  A BiCGStab step that breaks down (NaN residual) is
 * solved again with GMRES from the kept state, as in pfv_transport_advance (counted in pfv_stats.
 * advdiff_gmres_retries); a step whose AMG-preconditioned solve does not converge is restored from the kept state and
 * solved with Jacobi-GMRES (pfv_stats.advdiff_precond_fallbacks counts those).  Stops at the first step that still
 * does not converge (PFV_ERR_NOT_CONVERGED; steps_done counts the converged ones). */
pfv_status pfv_advdiff_advance(pfv_ctx* h, int n_steps, int method, double rtol, int maxit, double* c,
                               int32_t* steps_done, pfv_solve_info* last);
/* Total face flux (Nf) of the transported quantity for the state c (Nc), with q, w and bc_values of the last
 * pfv_advdiff_assemble: w q c_upstream (+ the Dirichlet-inflow / Neumann boundary parts) + flux_D c + bound_flux_D
 * bc_values.  Its divergence over a step equals source - accumulation o (c_new - c_old). */
pfv_status pfv_advdiff_face_flux(pfv_ctx* h, const double* c, double* out);

/* The adjoint of pfv_advdiff_advance (csrc/advdiff_adjoint.inc): every gradient of J = sum_{n=1..N} <g^n, c^n[obs_cells]>
 * through n_steps = N forward steps
 *     S c^n = acc o c^{n-1} - b_ref + b_D + src,      S = diag(acc) + div T_D + w div diag(q) U
 * of the system of the last pfv_advdiff_assemble (its q, w, bc_values, accumulation), which must be the active one
 * (else PFV_ERR_ARGUMENT).  For n = N .. 1 the call solves S^T lambda^n = g^n + acc o lambda^{n+1} (lambda^{N+1} = 0): the
 * values of S^T are taken on the pattern of S through transposed positions and (S^T, diag, rhs) is made the active
 * system ONCE; with PFV_PRECOND_AMG the hierarchy of S^T is set up by the first step and reused by all later ones.  Every
 * step is one pfv_solve started from lambda^{n+1} with the fallbacks of pfv_advdiff_advance: a BiCGStab step that breaks
 * down (NaN residual) is solved again with GMRES from the kept state, a step the AMG-preconditioned solve does not finish
 * with Jacobi-GMRES.  Then ONE pass over the faces and ONE over the cells accumulate the sums below; no step adds a host
 * read beyond those of its solve.
 *   loads [N][n_obs]: loads[n - 1] = g^n = dJ/dc^n on the observation cells obs_cells (n_obs int32 cell indices in HOST
 * memory, no repeats; NULL: every cell in order, n_obs must be Nc).  states (may be NULL): c^0 .. c^N as [N + 1][Nc]; one
 * slab is staged per step when they are host memory.  loads, states and the gradients follow
 * pfv_set_vectors_on_device; grad_flux_scale is one double in host memory.  method: PFV_SOLVE_BICGSTAB or
 * PFV_SOLVE_GMRES.
 *   With y^n_f = lambda^n[p] - lambda^n[m] (p / m the cells of cell_faces sign +1 / -1 at f, a missing cell contributes
 * nothing) and Lambda = sum_n lambda^n, each gradient may be NULL (not wanted):
 *     grad_c0 [Nc]               acc o lambda^1
 *     grad_source [Nc]           Lambda
 *     grad_bc_values [Nf]        -(B_D^T + (rhs_neu + rhs_dir diag(w q))^T) (cell_faces Lambda), zero off the boundary
 *     grad_accumulation [Nc]     sum_n lambda^n o (c^{n-1} - c^n)                                   (needs states)
 *     grad_flux [Nf]             -w sum_n y^n_f cup^n_f                                             (needs states)
 *     grad_flux_scale [1]        (1/w) sum_f q_f grad_flux_f, a reduction of fixed shape            (needs states)
 *     grad_conductivity [(3,3,Nc)]  sum_{e=(c,f)} zw_f dt_f/dK_rs(c), zw_f = -sum_n y^n_f w^n_f     (needs states)
 *     multipliers_out [N][Nc]    lambda^1 .. lambda^N
 * cup is the upwind value of pfv_transport_adjoint_multi: the upstream cell's c^n on interior and outflow faces,
 * bc_values on a Dirichlet inflow face, 0 on a Neumann face; grad_flux is the derivative at a FIXED upstream side.
 * w^n_f = filter_f (c^n difference) - dir_f sgn_f bc_f and dt_f/dK are those of pfv_flow_adjoint for p = c^n, mu =
 * lambda^n, and grad_conductivity has the meaning grad_perm has there: for pfv_tpfa_discretize it is the exact gradient of
 * the discrete problem; for pfv_mpfa_discretize it is the two-point product rule of the reference's AdTpfaFlux, NOT the
 * derivative of the MPFA matrices: that derivative is the grad_conductivity_exact of pfv_advdiff_adjoint_exact below.
 * All other gradients are exact for both schemes.  Nothing uses floating-point
 * atomics: two calls give the same bits.
 *   steps_done: the adjoint steps accepted.  A step that does not converge returns PFV_ERR_NOT_CONVERGED and writes NO
 * gradient.  last (may be NULL): the info of the last solve.
 *   After the call the handle holds NO active system and no advection-diffusion system (pfv_solve and
 * pfv_advdiff_advance ask for pfv_advdiff_assemble); the diffusion discretization, div T_D, b_D, the resident flux, the
 * flow order and the AMG aggregate maps are untouched.
 *   PFV_ERR_ARGUMENT: no active advection-diffusion system; another method; an obs_cells entry out of range or
 * repeated; a non-finite load (the text names the lowest index); grad_accumulation, grad_flux, grad_flux_scale or
 * grad_conductivity without states.  PFV_ERR_UNSUPPORTED: what pfv_advdiff_assemble refuses; Robin faces and faces
 * flagged PFV_BC_INTERNAL (the text names the first); a partial discretization with zeroed rows; PFV_PRECOND_SWEEP (the
 * substitution in reverse flow order on S^T is a later pull request); a pattern of div flux or bound_flux of 2^31
 * entries or more.  pfv_stats: advdiff_adjoint_*. */
pfv_status pfv_advdiff_adjoint(pfv_ctx* h, int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* loads,
                               const double* states, int method, double rtol, int maxit, double* grad_c0,
                               double* grad_source, double* grad_bc_values, double* grad_accumulation,
                               double* grad_flux, double* grad_flux_scale, double* grad_conductivity,
                               double* multipliers_out, int32_t* steps_done, pfv_solve_info* last);
/* The same call -- the same checks and refusals with the same status and text, the same solves, the same bits in every
 * output of pfv_advdiff_adjoint -- with one more output (csrc/mpfa_adjoint.inc, adj_batch_body):
 *     grad_conductivity_exact [(3,3,Nc)]  sum_{n=1..N} d/dK [ (z^n)^T (T_D c^n + B_D bc) ] at fixed c^n, bc,
 *                                  z^n_f = -y^n_f: the exact gradient of J with respect to the conductivity of the discrete
 *                                  problem, layout of perm_33n, all nine entries independent (on a 2-D grid only the
 *                                  2 x 2 block is non-zero); needs states; NULL: not formed, the call is
 *                                  pfv_advdiff_adjoint.
 * The conductivity enters a step only through div (T_D c^n + B_D bc), and y^n o c^n is not linear in a sum over n, so
 * every step needs its own solve of every interaction region; the region's geometry, its condensed matrix and its inverse
 * do not depend on n.  After an accepted step the call writes z^n into slab m of a ring of B = exact_batch slabs (0: the
 * default, 32; above N: N; negative: PFV_ERR_ARGUMENT) and notes c^n -- read in place when the states are device memory,
 * staged into a ring of B slabs when they are host memory.  Every B steps, and after the last step for what is pending,
 * ONE pass over the regions (one per wavefront) sets a region up and inverts it ONCE as pfv_flow_adjoint_exact does, then
 * runs that call's three stages per pending state with p = c^n, z = z^n and no vector source, the region's vectors reused
 * (the LDS need is that of pfv_flow_adjoint_exact).  The nd x nd numbers of a sub-cell start from the running sum in
 * memory (zeros before the first pass), stay in registers across the batch and take the states strictly in the order
 * n = N, N - 1, .., 1, each state's term summed from zero as in pfv_flow_adjoint_exact: the result has the same bits for
 * every B.  The cell sum of pfv_flow_adjoint_exact runs once, after the last pass.  No floating-point atomics; no step
 * adds a host read; the status words of the passes are read once, after the loop.  pfv_tpfa_discretize (the 1-D
 * delegate of MPFA included): grad_conductivity_exact = the two-point gradient, formed whether or not grad_conductivity
 * was asked for.  N = 0: zeros, no pass.
 *   Further statuses: PFV_ERR_ARGUMENT: grad_conductivity_exact without states, a negative exact_batch.
 * PFV_ERR_UNSUPPORTED names the node whose interaction region does not fit the LDS (found before the first solve);
 * PFV_ERR_SINGULAR names the node as pfv_mpfa_discretize does.  A refused or failed call writes no output.
 * pfv_stats: advdiff_adjoint_exact_* (and flow_adjoint_exact_map_* for the cell -> sub-cell map, kept with the sub-cell
 * topology and shared with pfv_flow_adjoint_exact). */
pfv_status pfv_advdiff_adjoint_exact(pfv_ctx* h, int n_steps, int64_t n_obs, const int32_t* obs_cells, const double* loads,
                                     const double* states, int method, double rtol, int maxit, double* grad_c0,
                                     double* grad_source, double* grad_bc_values, double* grad_accumulation,
                                     double* grad_flux, double* grad_flux_scale, double* grad_conductivity,
                                     double* multipliers_out, int32_t* steps_done, pfv_solve_info* last,
                                     double* grad_conductivity_exact, int exact_batch);
/* The resident face flux (pfv_mpfa_face_flux) of this handle: d_q (may be NULL) receives its device address -- Nf
 * doubles, valid until the next pfv_mpfa_face_flux or pfv_set_grid on the handle --, q_out (Nf, may be NULL) a copy,
 * in host or device memory as selected by pfv_set_vectors_on_device.  PFV_ERR_ARGUMENT when there is none. */
pfv_status pfv_resident_flux(pfv_ctx* h, double** d_q, double* q_out);

/* Device-pointer variants for multi-GPU drivers that keep vectors in HBM
 * (torch tensors): y = A x on the handle's stream; d_x has num_cols entries. */
pfv_status pfv_spmv_device(pfv_ctx* h, int which, const double* d_x, double* d_y);
/* same, but only rows [0, nrows): a sharded solve multiplies the rows of the cells a rank owns
 * (owned cells are numbered first) against owned + halo entries of x */
pfv_status pfv_spmv_device_rows(pfv_ctx* h, int which, int64_t nrows, const double* d_x, double* d_y);
pfv_status pfv_get_device_rhs(pfv_ctx* h, double** d_b, double** d_diag);
/* device-to-device copy of an internal vector into caller memory (e.g. a torch tensor):
 * which = 0 right-hand side, 1 diagonal of the system assembled last (Nc entries for flow,
 * nd Nc for mechanics) */
pfv_status pfv_copy_device_vector(pfv_ctx* h, int which, double* d_dst, int64_t count);
/* Block preconditioner of a sharded solve: aggregation-AMG hierarchy of the leading
 * n_own x n_own block of the active system (a rank's owned cells; couplings to halo columns are
 * dropped), then one V-cycle per call on device vectors of length n_own -- no communication
 * inside the preconditioner.  n_own = 0 means the whole active system. */
pfv_status pfv_amg_setup(pfv_ctx* h, int64_t n_own);
pfv_status pfv_amg_apply_device(pfv_ctx* h, const double* d_r, double* d_z);

/* Sharded Krylov solve: the fused BiCGStab / CG loop of pfv_solve on the rows of the cells this rank
 * owns (the leading n_own rows of the active system; owned cells are numbered first, the remaining
 * columns are halo cells owned by other ranks), with the two data exchanges of the distributed
 * method handed to the caller.  The reference has no distributed path; the split follows its
 * sub-problem machinery (numerics/fv/_fvutils.py:414-539), the solve stands in for
 * SolutionStrategy.solve_linear_system (models/solution_strategy.py:830-884).
 *   exchange_halo(user, d_x, stream): entries [n_own, n_local) of the SpMV input d_x are to be
 *     filled from their owners (RCCL ncclSend / ncclRecv over xGMI); the owned entries are current;
 *   allreduce_sum(user, d_vals, count, stream): in-place sum over the ranks of count (<= 8) doubles
 *     in device memory (ncclAllReduce) -- one call per fused group of dot products (BiCGStab: two calls per
 *     iteration, of 2 and 5 sums: the sums of the vector update ride with those of omega).
 * Both run on the calling thread between kernel launches and must only enqueue work ordered with
 * `stream` (the handle's hipStream_t as void*, see pfv_set_stream); a non-zero return aborts the
 * solve with PFV_ERR_ARGUMENT.  d_work: 2 * n_local + 8 doubles of caller device memory (the two
 * SpMV inputs d_x the hooks see are d_work and d_work + n_local, d_vals is d_work + 2 * n_local).
 * Preconditioner as selected by pfv_set_preconditioner: Jacobi, or one cycle of the block hierarchy
 * of pfv_amg_setup(n_own) (block Jacobi across ranks, no communication inside).  Every rank takes
 * the same branches: the convergence test reads the reduced residual.  d_x_owned receives n_own
 * values (device memory, zero start). */
typedef struct {
  int (*exchange_halo)(void* user, double* d_x, void* stream);
  int (*allreduce_sum)(void* user, double* d_vals, int count, void* stream);
  void* user;
  /* Transport of the coupled hierarchy (pfv_amg_setup_sharded; may be NULL for every other call).  The library
   * owns the halo plans of all levels and packs / unpacks itself; the transport only moves packed buffers:
   *   sendrecv(user, n_peers, peers, d_send, send_ptr, d_recv, recv_ptr, stream): to peer p go the doubles
   *     d_send[send_ptr[p] .. send_ptr[p+1]), from it arrive d_recv[recv_ptr[p] .. recv_ptr[p+1])
   *     (ncclGroupStart / ncclSend + ncclRecv per peer / ncclGroupEnd); the offset arrays are host memory, valid
   *     during the call only;
   *   allgather(user, d_send, d_recv, bytes_per_rank, stream): rank r's bytes_per_rank bytes land at
   *     d_recv + r * bytes_per_rank on every rank (ncclAllGather). */
  int (*sendrecv)(void* user, int n_peers, const int32_t* peers, const double* d_send, const int64_t* send_ptr,
                  double* d_recv, const int64_t* recv_ptr, void* stream);
  int (*allgather)(void* user, const void* d_send, void* d_recv, int64_t bytes_per_rank, void* stream);
} pfv_shard_hooks;
pfv_status pfv_solve_sharded(pfv_ctx* h, int method, double rtol, int maxit, int64_t n_own,
                             const pfv_shard_hooks* hooks, double* d_work, double* d_x_owned,
                             pfv_solve_info* info);

/* Coupled hierarchy of a sharded solve (instead of pfv_amg_setup(n_own), whose block hierarchy ignores the
 * couplings between ranks and pays for it in iterations): every level keeps the columns of the unknowns other ranks
 * own (aggregates never cross a rank boundary; the Galerkin product of the owned rows carries the halo columns
 * along, renamed to the owner's aggregates), smoothing and residual products see current halo values (one
 * point-to-point exchange before each), and from the first level with at most PFV_AMG_GATHER_ROWS (default 32768)
 * rows in total the rows of all ranks are gathered once (allgather) and every rank continues with the same
 * replicated hierarchy -- per cycle one allgather of that level's right-hand side, no further communication.
 * The plan of the finest level is given in CELLS (bs unknowns each travel): send_idx[send_ptr[p] ..) are the owned
 * cells peer p needs, in the order it expects them; recv_pos[recv_ptr[p] ..) the local cells (>= n_own / bs) its
 * values land in, in the order it sends them.  Every rank calls this (it is a collective of the transport);
 * the hooks (all four entries) must stay valid until the next setup or the handle's end.  The reference has no
 * distributed path (models/solution_strategy.py:830-884 solves on one process). */
pfv_status pfv_amg_setup_sharded(pfv_ctx* h, int64_t n_own, const pfv_shard_hooks* hooks, int rank, int world,
                                 int n_peers, const int32_t* peers, const int64_t* send_ptr,
                                 const int32_t* send_idx, const int64_t* recv_ptr, const int32_t* recv_pos);

/* The two hooks served natively over RCCL (xGMI), no Python in the iteration (csrc/rccl_hooks.inc):
 * pack kernel -> ncclGroupStart / ncclSend + ncclRecv per neighbour / ncclGroupEnd -> unpack kernel, and
 * ncclAllReduce of the fused pair of sums, all enqueued on the handle's stream.  librccl is bound with
 * dlopen at the first call.  Rank 0 creates the id, the caller distributes its 128 bytes (torch.distributed,
 * MPI, a file), every rank creates its communicator on its handle's device and describes its halo plan;
 * pfv_rccl_hooks then fills the struct pfv_solve_sharded takes.  PFV_ERR_UNSUPPORTED from the host-emulation
 * build or when librccl cannot be loaded. */
typedef struct pfv_rccl_comm pfv_rccl_comm;
pfv_status pfv_rccl_unique_id(char* id128);
pfv_status pfv_rccl_comm_create(pfv_ctx* h, const char* id128, int rank, int world, pfv_rccl_comm** out);
pfv_status pfv_rccl_set_halo_plan(pfv_rccl_comm* c, int n_peers, const int32_t* peers, const int64_t* send_ptr,
                                  const int32_t* send_idx, const int64_t* recv_ptr, const int32_t* recv_pos);
pfv_status pfv_rccl_hooks(pfv_rccl_comm* c, pfv_shard_hooks* out);
pfv_status pfv_rccl_stats(pfv_rccl_comm* c, int64_t* exchanges, int64_t* allreduces, int64_t* bytes_per_exchange);
const char* pfv_rccl_last_error(pfv_rccl_comm* c);
void pfv_rccl_comm_destroy(pfv_rccl_comm* c);

/* ---- Device-resident CSR matrices and the sparse algebra of the step after discretize --------
 * What MergedOperator.parse (numerics/ad/ad_utils.py:597-663 -> matrix_operations.csr_matrix_from_sparse_blocks) and the
 * scipy products / sums of the operator tree (assembled by EquationSystem.assemble, numerics/ad/equation_system.py:1579)
 * do on the host, kept in HBM: a pfv_csr is created from a discretization matrix of a handle without a host copy
 * (pfv_csr_from_matrix) or uploaded once (projections, divergences: pfv_csr_from_host), combined block-diagonally, by
 * products and by sums, and handed to pfv_solve as the active system (pfv_csr_set_system).  scipy's conventions, so
 * that results compare entry by entry: rows sorted by column without duplicates (required of inputs, guaranteed of
 * outputs), accumulation in the order of csr_matmat / csr_binop_csr with every product rounded on its own (same bits),
 * entries that come out exactly zero are not stored.  A pfv_csr belongs to the handle it was created on (same
 * device for all operands) and must be freed before that handle is destroyed. */
typedef struct pfv_csr pfv_csr;
/* indptr is checked on the host before anything is uploaded (indptr[0] = 0, non-decreasing, every entry within
 * [0, nnz = indptr[nrows]]), the rows on the device (sorted by column, no duplicates, 0 <= column < ncols):
 * PFV_ERR_ARGUMENT otherwise */
pfv_status pfv_csr_from_host(pfv_ctx* h, int64_t nrows, int64_t ncols, const int32_t* indptr, const int32_t* indices,
                             const double* values, pfv_csr** out);
/* device-to-device copy of matrix `which` (pfv_matrix_id) of handle src */
pfv_status pfv_csr_from_matrix(pfv_ctx* h, pfv_ctx* src, int which, pfv_csr** out);
pfv_status pfv_csr_block_diag(pfv_ctx* h, int n, const pfv_csr* const* blocks, pfv_csr** out);
pfv_status pfv_csr_matmul(pfv_ctx* h, const pfv_csr* A, const pfv_csr* B, pfv_csr** out);   /* A B (rows fed by more than
                                                     4096 products take a slower path through global sorts) */
pfv_status pfv_csr_axpby(pfv_ctx* h, double alpha, const pfv_csr* A, double beta, const pfv_csr* B, pfv_csr** out);
pfv_status pfv_csr_transpose(pfv_ctx* h, const pfv_csr* A, pfv_csr** out);
/* scipy.sparse.bmat: nbr x nbc blocks, row-major, NULL = zero block of row_sizes[i] x col_sizes[j] */
pfv_status pfv_csr_bmat(pfv_ctx* h, int nbr, int nbc, const pfv_csr* const* blocks, const int64_t* row_sizes,
                        const int64_t* col_sizes, pfv_csr** out);
pfv_status pfv_csr_scale(pfv_csr* A, const double* row_scale, const double* col_scale);   /* in place; host arrays or NULL */
pfv_status pfv_csr_divide(pfv_csr* A, double s);   /* in place, scipy's A / s: every value MULTIPLIED by the rounded
                                                      reciprocal 1.0 / s (scipy's _divide is _mul_scalar(1. / s)), which
                                                      differs from a true division in the last bit */
pfv_status pfv_csr_spmv(const pfv_csr* A, const double* x, double* y);                     /* host vectors */
pfv_status pfv_csr_spmv_device(const pfv_csr* A, const double* d_x, double* d_y);
pfv_status pfv_csr_info(const pfv_csr* A, int64_t* nrows, int64_t* ncols, int64_t* nnz);
pfv_status pfv_csr_get(const pfv_csr* A, int32_t* indptr, int32_t* indices, double* values);  /* any may be NULL */
/* (A, rhs) become the active system of h -- what pfv_solve / pfv_amg_setup work on -- without leaving the device */
pfv_status pfv_csr_set_system(pfv_ctx* h, const pfv_csr* A, const double* rhs, int rhs_on_device);
void pfv_csr_free(pfv_csr* A);

/* run this handle's work on an externally owned HIP stream (hipStream_t passed as void*, e.g.
 * torch.cuda.current_stream().cuda_stream) so that it is ordered with the caller's kernels and
 * RCCL collectives.  NULL is the legacy default stream (what torch's default stream is) -- the
 * handle's own stream is non-blocking and is NOT ordered with it; pfv_reset_stream goes back to
 * the handle's own stream. */
pfv_status pfv_set_stream(pfv_ctx* h, void* hip_stream);
pfv_status pfv_reset_stream(pfv_ctx* h);
pfv_status pfv_sync(pfv_ctx* h);

pfv_status pfv_get_stats(pfv_ctx* h, pfv_stats* out);
/* the same for a caller compiled against another revision of this header: writes at most `struct_size` bytes
 * (= the caller's sizeof(pfv_stats); fields are only ever appended), so a shorter struct is never overrun */
pfv_status pfv_get_stats_n(pfv_ctx* h, void* out, size_t struct_size);

/* Measurement hook for bench.py: average duration (ms, HIP events on the handle's stream)
 * of `reps` back-to-back launches of one kernel on the data currently in the handle.
 * kernel: 0 = CSR SpMV with A, 1 = interaction-region (node) kernel, 2 = face kernel,
 * 3 = AMG smoothing product, 4 = stream triad (no discretization needed). */
enum { PFV_KERNEL_SPMV_A = 0, PFV_KERNEL_NODE = 1, PFV_KERNEL_FACE = 2,
       PFV_KERNEL_AMG_SMOOTH = 3, /* finest-level smoothing product of the AMG cycle (needs a built hierarchy) */
       PFV_KERNEL_TRIAD = 4,      /* a = b + s c on 3 x 2^27 doubles (3.2 GB moved per launch): the measured
                                     device bandwidth next to the data-sheet 8 TB/s (SURVEY 8(d) "Metric") */
       PFV_KERNEL_READ = 5        /* read-only stream over 2^28 doubles (2.1 GB): the ceiling of the read-dominated
                                     SpMV kernels */ };
pfv_status pfv_time_kernel(pfv_ctx* h, int kernel, int reps, double* avg_ms);

/* Test hook: copy the leading `count` entries of an internal FP64 device array to the host (0 = the
 * per-node response tables, 1 = the boundary columns of the nodes on the boundary). */
pfv_status pfv_debug_copy(pfv_ctx* h, int which, double* dst, int64_t count);

/* Test hook: the integer arrays and scalars of the sub-cell topology on the handle.  `which` names the array, in this
 * order: 0 node_hptr (i32), 1 h_cell (i32), 2 h_lf (u8), 3 h_sgn (i8), 4 h_first (u8), 5 node_fptr (i32), 6 node_sf (i32),
 * 7 sf_face (i32), 8 sf_ls (u8), 9 face_nsides (i32), 10 node_face (i32), 11 node_bptr (i32), 12 node_bfaces (i32),
 * 13 node_bls (u8), 14 node_tptr (i64), 15 node_tbptr (i64), 16 node_cells (i32), 17 face_order (i32),
 * 18 node_order (i32), 19 class_begin (i64), 20 the scalars as 17 x i64 (nh, max_face_nodes, max_cell_faces, max_block,
 * max_deg, max_bnd_per_node, sum_block_sq, tab_len, tabb_len, the bits of stats.node_flops, stats.num_nodes,
 * stats.num_sub_half_faces, stats.sum_block_sq, stats.max_block, stats.node_table_doubles, the topology digest, the construction that ran: 1 node-cooperative, 0 reference).
 * *bytes receives the size of the array in bytes; it is copied to dst when dst is not NULL and capacity >= *bytes. */
pfv_status pfv_debug_topology(pfv_ctx* h, int which, void* dst, int64_t capacity, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* POREFV_H */
