"""``AdvectionDiffusion`` — upwind advection plus MPFA / TPFA diffusion of one keyword as ONE device system with an
implicit Euler step that stays in HBM (csrc/advdiff.inc).  It reads ``data[PARAMETERS][keyword]`` as the reference's
pair ``pp.Mpfa(keyword)`` + ``pp.Upwind(keyword)`` would read one dictionary: ``second_order_tensor``, ``bc``,
``bc_values``, ``darcy_flux`` (an array, or a ``ResidentFlux`` of any handle on the device) and, beyond the reference,
``flux_scale`` (a positive scalar ``w``, default 1: the fluid heat capacity and the like, so that a resident Darcy flux
need not be rescaled).

The class takes host arrays.  The resident flux of the shared handle is read in place; that of another handle -- the
flow handle, usually -- is copied through the host once per assembly.  ``Context.advdiff_assemble(device=True,
q_device_ptr=other.resident_flux_ptr())`` with ``Context.advdiff_advance(device=True)`` keeps every vector in HBM.

Sign convention (next to the note in upwind.py): with ``(A_D, b_D)`` what ``Mpfa.assemble_matrix_rhs`` returns -- a
solver right-hand side, ``b_D = -div @ bound_flux @ bc_values`` -- and ``(A_U, b_ref)`` what ``Upwind.
assemble_matrix_rhs`` returns for the flux ``w q`` -- ``b_ref`` the boundary part of the flux divergence, not a
right-hand side --, ``assemble_matrix_rhs`` here returns ``A = A_D + A_U(w q) = A_D + w A_U(q)`` and
``b = b_D - b_ref``: the steady balance is ``A c = b + source``, and ``solve`` / ``advance`` solve
``(diag(acc) + A) c = acc * c_old + b + source``."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sps

from . import _lib
from .params import PARAMETERS
from .upwind import ResidentFlux


class AdvectionDiffusion:
    """Advection-diffusion of ``keyword`` on the device.  ``diffusion``: the ``Mpfa`` / ``Tpfa`` object of the keyword
    whose device handle of a grid is shared (None: one is made, ``scheme`` = "mpfa" or "tpfa")."""

    def __init__(self, keyword: str = "transport", diffusion=None, scheme: str = "mpfa", device: int = 0, library=None):
        if diffusion is None:
            from .mpfa import Mpfa
            from .tpfa import Tpfa

            if scheme not in ("mpfa", "tpfa"):
                raise ValueError('scheme must be "mpfa" or "tpfa"')
            diffusion = (Mpfa if scheme == "mpfa" else Tpfa)(keyword, device, library)
        elif diffusion.keyword != keyword:
            raise ValueError("the diffusion discretization must be one of the same keyword")
        self.keyword = keyword
        self.diffusion = diffusion
        self.device = device
        self._library = library
        self._flux_array_key = "darcy_flux"

    @property
    def flux_array_key(self) -> str:
        return self._flux_array_key

    @flux_array_key.setter
    def flux_array_key(self, value: str) -> None:
        self._flux_array_key = value

    def ndof(self, sd) -> int:
        return sd.num_cells

    def context(self, sd) -> _lib.Context:
        if hasattr(sd, "periodic_face_map"):
            raise _lib.PorefvError(5, "advection-diffusion on periodic grids is not covered")
        if sd.dim < 2 and hasattr(self.diffusion, "_tpfa"):  # (Mpfa hands 1-D grids to its Tpfa object)
            return self.diffusion._tpfa().context(sd)
        return self.diffusion.context(sd)

    # ---- parameters ---------------------------------------------------------------------
    def _flux(self, sd, pd):
        """The flux parameter: a host array of Nf values, None for the resident flux of the shared handle, or the
        ``Context`` of another handle whose resident flux is meant."""
        q = pd.get(self._flux_array_key, None)
        if q is None:
            raise KeyError(self._flux_array_key)
        if isinstance(q, ResidentFlux):
            if q.context is self.context(sd):
                return None
            if q.context.nf != sd.num_faces:
                raise ValueError("the resident flux belongs to another grid")
            return q.context
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (sd.num_faces,):
            raise ValueError(f"the flux array must have one entry per face ({sd.num_faces}), not shape {q.shape}")
        return q

    def _scale(self, pd) -> float:
        w = float(pd.get("flux_scale", 1.0))
        if not (w > 0.0 and np.isfinite(w)):
            raise ValueError("flux_scale must be positive and finite")
        return w

    def _check(self, sd, pd):
        if int(pd.get("num_components", 1)) != 1:
            raise ValueError("Dimension mismatch in assembly of discretization term: advection-diffusion takes "
                             "num_components = 1")

    # ---- discretization and assembly ------------------------------------------------------
    def discretize(self, sd, data: dict) -> None:
        """The diffusion discretization of the keyword (its six matrices go to ``data`` as ``Mpfa.discretize`` leaves
        them); the upwind part needs none: the upstream side is decided from the flux in every assembly."""
        pd = data[PARAMETERS][self.keyword]
        self._check(sd, pd)
        if sd.dim > 0:
            self.context(sd)  # (periodic grids are refused before anything is computed)
        self.diffusion.discretize(sd, data)

    def _assemble(self, sd, data, accumulation=None, c_old=None, source=None, bound_rhs=False, bc=True):
        pd = data[PARAMETERS][self.keyword]
        self._check(sd, pd)
        ctx = self.context(sd)
        q = self._flux(sd, pd)
        if isinstance(q, _lib.Context):
            # the vectors of this call are host arrays, so the other handle's flux comes as one too (Nf doubles down and
            # up again per assembly); Context.advdiff_assemble(device=True, q_device_ptr=...) takes it in place
            q = q.resident_flux()
        bv = np.asarray(pd["bc_values"], dtype=float) if bc else None
        try:
            return ctx.advdiff_assemble(bv, q, self._scale(pd), accumulation, c_old, source, bound_rhs=bound_rhs)
        except _lib.PorefvError as e:
            if e.status == 4:
                raise ValueError(e.message) from None
            raise

    def assemble_matrix_rhs(self, sd, data: dict):
        """``(A, b)`` with ``A = A_D + w A_U`` and ``b = b_D - b_ref`` (module text): ``A c = b + source``."""
        if sd.dim == 0:
            return sps.csr_matrix((sd.num_cells, sd.num_cells)), np.zeros(sd.num_cells)
        self._assemble(sd, data)
        ctx = self.context(sd)
        return ctx.matrix(_lib.MAT_ADVDIFF_SYSTEM), ctx.rhs()

    def update_flux(self, sd, data: dict, accumulation=None, c_old=None, source=None) -> None:
        """A new flux (``darcy_flux`` / ``flux_scale`` of ``data``) on the same discretization: the values of the
        system, its diagonal and the right-hand side are refreshed; nothing symbolic runs and the boundary values of
        the last assembly stand."""
        self._assemble(sd, data, accumulation, c_old, source, bc=False)

    def solve(self, sd, data: dict, accumulation=None, c_old=None, source=None, method: str = "bicgstab",
              precond: str = "amg", rtol: float = 1e-12, maxit: int = 20000, x0=None, restart: int = 0):
        """Solve ``(diag(accumulation) + A) c = accumulation * c_old + b + source``.  Returns (c, info).

        ``precond="sweep"``: downstream-ordered Gauss-Seidel, one substitution in the flow order of ``darcy_flux``
        (``context(sd).sweep_info()``).  For this system it is always a preconditioner of ``method``, never exact: the
        diffusion couples every cell to its downstream neighbours too.  It pays in the advection-dominated regime."""
        self._assemble(sd, data, accumulation, c_old, source)
        return self.context(sd).solve(method=method, rtol=rtol, maxit=maxit, x0=x0, restart=restart, precond=precond)

    def advance(self, sd, data: dict, c0, n_steps: int, accumulation, source=None, method: str = "bicgstab",
                precond: str = "amg", rtol: float = 1e-12, maxit: int = 20000, raise_on_fail: bool = True,
                return_states: bool = False):
        """``n_steps`` implicit Euler steps from ``c0`` with ``accumulation`` = capacity x volume / dt per cell, all on
        the device, preconditioned by ``precond`` ("amg": one hierarchy for all steps; "jacobi"; "sweep": the
        substitution in flow order, built once per flux -- a preconditioner here, see ``solve``).  Returns (c_n, info);
        info["steps_done"] counts the converged steps.  ``context(sd).stats()`` has ``advdiff_iterations`` and
        ``advdiff_precond_fallbacks`` (steps the AMG- or sweep-preconditioned solve left to Jacobi-GMRES).

        ``return_states``: returns (c_n, info, states) with states = c^0 .. c^N as (N + 1, Nc) -- what ``adjoint`` takes
        --, produced by stepping one step at a time on the same assembly (the statistics are then those of the last
        step; info["steps_done"] and info["iterations"] are summed; the slabs after a step that failed are NaN)."""
        self._assemble(sd, data, accumulation, None, source)
        ctx = self.context(sd)
        if not return_states:
            return ctx.advdiff_advance(c0, n_steps, method=method, rtol=rtol, maxit=maxit, precond=precond,
                                       raise_on_fail=raise_on_fail)
        c = np.array(c0, dtype=np.float64, copy=True).ravel()
        states = np.full((int(n_steps) + 1, ctx.nc), np.nan)
        if c.shape != (ctx.nc,):
            raise ValueError("c0 must have one entry per cell")
        states[0] = c
        total = {"steps_done": 0, "iterations": 0, "converged": True, "rel_residual": 0.0, "solve_ms": 0.0}
        for n in range(int(n_steps)):
            c, info = ctx.advdiff_advance(c, 1, method=method, rtol=rtol, maxit=maxit, precond=precond,
                                          raise_on_fail=raise_on_fail)
            total = dict(info, steps_done=total["steps_done"] + info["steps_done"],
                         iterations=total["iterations"] + info["iterations"])
            if info["steps_done"] != 1:
                break
            states[n + 1] = c
        return c, total, states

    def adjoint(self, sd, data: dict, n_steps: int, accumulation, loads, states, obs_cells=None, source=None,
                want=("c0", "source", "bc_values"), method: str = "bicgstab", precond: str = "amg",
                rtol: float = 1e-12, maxit: int = 20000, raise_on_fail: bool = True, exact_batch=None):
        """The adjoint of ``advance``: the gradients of ``J = sum_{n=1..N} <loads[n-1], c^n[obs_cells]>`` through
        ``n_steps`` = N steps ``S c^n = acc o c^{n-1} - b_ref + b_D + source`` (csrc/advdiff_adjoint.inc).  The system is
        assembled exactly as ``advance`` assembles it; then, backwards in time, ``S^T lambda^n = g^n + acc o lambda^{n+1}``
        is one transposed Krylov solve per step, preconditioned by ``precond`` ("amg": one hierarchy of S^T for all steps;
        "jacobi"), with the fallbacks of ``advance``.

        ``loads``: (N, n_obs); ``obs_cells``: n_obs cell indices without repeats, or None (every cell in order);
        ``states``: c^0 .. c^N as (N + 1, Nc) -- ``advance(..., return_states=True)`` -- or None.  With
        ``y^n_f = lambda^n[p] - lambda^n[m]`` (p / m the cells of ``cell_faces`` sign +1 / -1 at face f; a missing cell
        contributes nothing) and ``Lambda = sum_n lambda^n``, ``want`` names

        ================  ========  ======================================================================
        "c0"              Nc        ``acc o lambda^1``
        "source"          Nc        ``Lambda``
        "accumulation"    Nc        ``sum_n lambda^n o (c^{n-1} - c^n)``                       (needs states)
        "bc_values"       Nf        ``-(B_D^T + (rhs_neu + rhs_dir diag(w q))^T)(cell_faces Lambda)``; zero off the
                                    boundary
        "flux"            Nf        ``-w sum_n y^n_f cup^n_f``, cup the upwind value: upstream ``c^n`` on interior
                                    and outflow faces, ``bc_values`` on a Dirichlet inflow face, 0 on a Neumann face;
                                    the derivative at a fixed upstream side                   (needs states)
        "flux_scale"      float     ``(1/w) sum_f q_f grad_flux_f``                            (needs states)
        "conductivity"    3,3,Nc    ``sum_e zw_f dt_f/dK_rs(c)``, ``zw_f = -sum_n y^n_f w^n_f`` with the face weight
                                    ``w^n_f`` and the two-point ``dt_f/dK`` of ``adjoint_flow``  (needs states)
        "conductivity_exact"  3,3,Nc  ``sum_n d/dK [(z^n)^T (T_D c^n + B_D bc)]`` at fixed ``c^n``, ``z^n = -y^n``: the
                                    derivative of the MPFA matrices themselves                (needs states)
        "multipliers"     N,Nc      every ``lambda^n``
        ================  ========  ======================================================================

        "conductivity" has the meaning ``grad_perm`` has in ``adjoint_flow``: it is exact for a TPFA diffusion; for MPFA
        it is the two-point product rule of ``AdTpfaFlux``, NOT the derivative of the MPFA matrices.  That derivative is
        "conductivity_exact" (``Context.ADVDIFF_ADJOINT_EXACT``; pfv_advdiff_adjoint_exact, csrc/mpfa_adjoint.inc): the
        exact gradient of the discrete problem with respect to the tensor of every cell, all nine entries independent --
        one pass over the interaction regions per ``exact_batch`` steps (None: the library's default), each region set up
        and inverted once per pass; the bits do not depend on ``exact_batch``.  For a TPFA diffusion (a 1-D grid
        included) it has the bits of "conductivity".  All other gradients are exact for both schemes.  ``grads["flux"]`` is what ``Mpfa.adjoint_flow(..., grad_flux=grads["flux"])`` /
        ``Tpfa.adjoint_flow`` of the flow problem that produced ``darcy_flux`` takes: the chain ends at the permeability
        of the flow.

        Returns (grads, info); info["steps_done"] counts the accepted steps; a step that does not converge leaves the
        gradients zero.  Afterwards the handle holds no assembled system.  ``context(sd).stats()`` has
        ``advdiff_adjoint_*``."""
        self._assemble(sd, data, accumulation, None, source)
        try:
            return self.context(sd).advdiff_adjoint(n_steps, loads, states=states, obs_cells=obs_cells, want=want,
                                                    method=method, rtol=rtol, maxit=maxit, precond=precond,
                                                    raise_on_fail=raise_on_fail,
                                                    exact_batch=0 if exact_batch is None else exact_batch)
        except _lib.PorefvError as e:
            if e.status == 4:
                raise ValueError(e.message) from None
            raise

    def total_flux(self, sd, data: dict, c) -> np.ndarray:
        """Total face flux of the transported quantity for the state ``c``, with the flux and boundary values of the
        last assembly: ``w q c_upstream`` (+ boundary parts) ``+ flux_D c + bound_flux_D bc_values``."""
        return self.context(sd).advdiff_face_flux(c)
