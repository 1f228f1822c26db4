"""``Upwind`` — first-order upwind advection on the device with the operator API of the reference's
``pp.Upwind`` (numerics/fv/upwind.py:15-375): same keys, same stored patterns, and beyond it a transport
solve and implicit Euler stepping that stay in HBM (csrc/upwind.inc).

Sign convention of ``assemble_matrix_rhs`` (the reference's): it returns ``(A, b_ref)`` with
``A = div @ diag(q) @ U`` and ``b_ref = div @ (rhs_neu + rhs_dir @ diag(q)) @ bc_values``, the boundary part of the
flux divergence -- not a solver right-hand side.  The balance reads ``acc * (c - c_old) + A c + b_ref = source``;
``solve`` / ``advance`` solve ``(diag(acc) + A) c = acc * c_old - b_ref + source``."""
from __future__ import annotations

import contextlib

import numpy as np
import scipy.sparse as sps

from . import _lib
from .grid import grid_to_raw
from .params import DISCRETIZATION_MATRICES, PARAMETERS, bc_flags


def per_component(name, a, k, n):
    """``a`` as a (k, n) array: one row shared by the k components, or a row for each"""
    a = np.asarray(a, dtype=np.float64)
    if a.shape == (n,):
        return np.broadcast_to(a, (k, n))
    if a.shape != (k, n):
        raise ValueError(f"{name} must have shape ({n},) or ({k}, {n}), not {a.shape}")
    return a


@contextlib.contextmanager
def _argument_errors(with_state=False):
    """An argument the library refuses (status 4) is a ValueError with the library's words; ``with_state``: it carries
    the ``state`` and ``info`` of the library's error."""
    try:
        yield
    except _lib.PorefvError as e:
        if e.status != 4:
            raise
        err = ValueError(e.message)
        if with_state:
            err.state, err.info = getattr(e, "state", None), getattr(e, "info", None)
        raise err from None


class ResidentFlux:
    """Stands for the face flux kept on a device handle (``Mpfa.darcy_flux(..., resident=True)``): put it where the
    flux array goes, ``data[PARAMETERS][keyword]["darcy_flux"]``, and ``Upwind(flow=...)`` reads the flux in HBM."""

    def __init__(self, context):
        self.context = context

    def __repr__(self):
        return "ResidentFlux(<device handle>)"


def flow_darcy_flux(ctx, pd: dict, p, vector_source=None, resident: bool = False):
    """Face flux of the flow discretization on ``ctx`` for the cell pressures ``p``."""
    q = ctx.face_flux(p, np.asarray(pd["bc_values"], dtype=float), vector_source, out=not resident)
    return ResidentFlux(ctx) if resident else q


class CoreyFractionalFlow:
    """Fractional flow of the wetting phase with Corey relative permeabilities: ``s_e = clip((s - s_wr) /
    (1 - s_wr - s_nr), 0, 1)``, ``f = l_w / (l_w + l_n)`` with ``l_w = s_e**n_w / mu_w``, ``l_n = (1 - s_e)**n_n / mu_n``.
    Calling it evaluates the curve with numpy -- the curve ``Upwind.advance_saturation`` steps with on the device."""

    kind = _lib.FLUXFN_COREY

    def __init__(self, s_wr=0.0, s_nr=0.0, n_w=2.0, n_n=2.0, mu_w=1.0, mu_n=1.0):
        self.s_wr, self.s_nr, self.n_w, self.n_n = float(s_wr), float(s_nr), float(n_w), float(n_n)
        self.mu_w, self.mu_n = float(mu_w), float(mu_n)

    @property
    def params(self) -> np.ndarray:
        return np.array([self.s_wr, self.s_nr, self.n_w, self.n_n, self.mu_w, self.mu_n])

    def __call__(self, s):
        se = np.clip((np.asarray(s, dtype=np.float64) - self.s_wr) / (1.0 - self.s_wr - self.s_nr), 0.0, 1.0)
        lw, ln = se ** self.n_w / self.mu_w, (1.0 - se) ** self.n_n / self.mu_n
        return lw / (lw + ln)

    def __repr__(self):
        return (f"CoreyFractionalFlow(s_wr={self.s_wr}, s_nr={self.s_nr}, n_w={self.n_w}, n_n={self.n_n}, "
                f"mu_w={self.mu_w}, mu_n={self.mu_n})")


class TabulatedFractionalFlow:
    """Piecewise-linear flux function through ``values`` (2 .. 1024 of them, finite, nondecreasing) on uniform knots
    over [0, 1].  Calling it evaluates the curve with numpy."""

    kind = _lib.FLUXFN_TABLE

    def __init__(self, values):
        self.values = np.array(values, dtype=np.float64).ravel()

    @property
    def params(self) -> np.ndarray:
        return self.values

    def __call__(self, s):
        s = np.clip(np.asarray(s, dtype=np.float64), 0.0, 1.0)
        return np.interp(s, np.linspace(0.0, 1.0, self.values.size), self.values)

    def __repr__(self):
        return f"TabulatedFractionalFlow(<{self.values.size} values>)"


class LinearIsotherm:
    """Linear sorption isotherm ``S = kd c`` (``kd >= 0``).  Calling it evaluates the curve with numpy -- the curve
    ``Upwind.advance_sorbing_components`` steps with on the device."""

    kind = _lib.ISOTHERM_LINEAR

    def __init__(self, kd=1.0):
        self.kd = float(kd)

    def params(self) -> np.ndarray:
        return np.array([self.kd, 0.0])

    def __call__(self, c):
        return self.kd * np.asarray(c, dtype=np.float64)

    def __repr__(self):
        return f"LinearIsotherm(kd={self.kd})"


class FreundlichIsotherm:
    """Freundlich sorption isotherm ``S = kf c**n`` for ``c >= 0`` (``kf >= 0``, ``n > 0``; ``n < 1`` has an infinite slope
    at 0).  Calling it evaluates the curve with numpy."""

    kind = _lib.ISOTHERM_FREUNDLICH

    def __init__(self, kf=1.0, n=1.0):
        self.kf, self.n = float(kf), float(n)

    def params(self) -> np.ndarray:
        return np.array([self.kf, self.n])

    def __call__(self, c):
        return self.kf * np.asarray(c, dtype=np.float64) ** self.n

    def __repr__(self):
        return f"FreundlichIsotherm(kf={self.kf}, n={self.n})"


class LangmuirIsotherm:
    """Langmuir sorption isotherm ``S = q_max b c / (1 + b c)`` for ``c >= 0`` (``q_max >= 0``, ``b >= 0``).  Calling it
    evaluates the curve with numpy."""

    kind = _lib.ISOTHERM_LANGMUIR

    def __init__(self, q_max=1.0, b=1.0):
        self.q_max, self.b = float(q_max), float(b)

    def params(self) -> np.ndarray:
        return np.array([self.q_max, self.b])

    def __call__(self, c):
        c = np.asarray(c, dtype=np.float64)
        return self.q_max * self.b * c / (1.0 + self.b * c)

    def __repr__(self):
        return f"LangmuirIsotherm(q_max={self.q_max}, b={self.b})"


class Upwind:
    """Upwind discretization of ``keyword`` on the device.  ``flow``: an ``Mpfa`` / ``Tpfa`` object whose device
    handle of a grid is shared, so that the flux it left resident can be taken without a copy."""

    def __init__(self, keyword: str = "transport", device: int = 0, library=None, flow=None):
        self.keyword = keyword
        self.device = device
        self._library = library
        self._flow = flow
        self.upwind_matrix_key = "transport"
        self.bound_transport_dir_matrix_key = "rhs_dir"
        self.bound_transport_neu_matrix_key = "rhs_neu"
        self._flux_array_key = "darcy_flux"
        self._contexts: dict = {}

    @property
    def flux_array_key(self) -> str:
        return self._flux_array_key

    @flux_array_key.setter
    def flux_array_key(self, value: str) -> None:
        self._flux_array_key = value

    def ndof(self, sd) -> int:
        return sd.num_cells

    def context(self, sd) -> _lib.Context:
        if self._flow is not None:
            if hasattr(sd, "periodic_face_map"):
                raise _lib.PorefvError(5, "upwind on periodic grids is not covered")
            if sd.dim < 2 and hasattr(self._flow, "_tpfa"):  # (Mpfa hands 1-D grids to its Tpfa object)
                return self._flow._tpfa().context(sd)
            return self._flow.context(sd)
        ent = self._contexts.get(id(sd))
        if ent is None or ent[0] is not sd:
            if hasattr(sd, "periodic_face_map"):
                raise _lib.PorefvError(5, "upwind on periodic grids is not covered")
            ctx = _lib.Context(self.device, self._library)
            ctx.set_grid(grid_to_raw(sd))
            self._contexts[id(sd)] = (sd, ctx)
            return ctx
        return ent[1]

    # ---- the reference's API ---------------------------------------------------------
    def _flux(self, sd, pd):
        """The flux parameter: None for the resident one, else an array of Nf values."""
        q = pd.get(self._flux_array_key, None)
        if q is None or isinstance(q, ResidentFlux):
            if self._flow is None and q is None:
                raise KeyError(self._flux_array_key)
            if isinstance(q, ResidentFlux) and q.context is not self.context(sd):
                raise ValueError("the resident flux lives on another device handle: pass flow=<its discretization>")
            return None
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (sd.num_faces,):
            raise ValueError(f"the flux array must have one entry per face ({sd.num_faces}), not shape {q.shape}")
        return q

    def discretize(self, sd, data: dict) -> None:
        pd = data[PARAMETERS][self.keyword]
        md = data.setdefault(DISCRETIZATION_MATRICES, {}).setdefault(self.keyword, {})
        if sd.dim == 0:
            md[self.upwind_matrix_key] = sps.csr_matrix((0, 1))
            md[self.bound_transport_dir_matrix_key] = sps.csr_matrix((0, 0))
            md[self.bound_transport_neu_matrix_key] = sps.csr_matrix((0, 0))
            return
        k = int(pd.get("num_components", 1))
        if k < 1:
            raise ValueError("num_components must be at least 1")
        q = self._flux(sd, pd)
        ctx = self.context(sd)
        ctx.upwind_set_bc(bc_flags(pd["bc"]) if "bc" in pd else None)
        with _argument_errors():  # (the reference fails in scipy's coo -> csr conversion with the same words)
            ctx.upwind_discretize(q, k)
        for key, which in ((self.upwind_matrix_key, _lib.MAT_UPWIND),
                           (self.bound_transport_dir_matrix_key, _lib.MAT_UPWIND_RHS_DIR),
                           (self.bound_transport_neu_matrix_key, _lib.MAT_UPWIND_RHS_NEU)):
            md[key] = ctx.matrix(which)

    def _assemble(self, sd, data, accumulation=None, c_old=None, source=None, bound_rhs=False):
        pd = data[PARAMETERS][self.keyword]
        ctx = self.context(sd)
        with _argument_errors():
            return ctx.upwind_assemble(np.asarray(pd["bc_values"], dtype=float), self._flux(sd, pd), accumulation, c_old,
                                       source, bound_rhs=bound_rhs)

    def assemble_matrix_rhs(self, sd, data: dict):
        """``(A, b_ref)`` as the reference returns them (see the module text for the sign of ``b_ref``)."""
        b = self._assemble(sd, data, bound_rhs=True)
        return self.context(sd).matrix(_lib.MAT_TRANSPORT_SYSTEM), b

    def darcy_flux(self, sd, beta, cell_apertures=None) -> np.ndarray:
        """Flux of a constant velocity ``beta`` (3 values) through every face: ``beta . n_f`` with the area-weighted
        normals of the grid, times the face aperture -- the mean of ``cell_apertures`` over the one or two cells of the
        face, 1 where none are given.  One value per face (a point grid without faces gives an empty array)."""
        vel = np.asarray(beta, dtype=np.float64).reshape(-1)
        if vel.shape != (3,):
            raise ValueError("beta must hold the three components of the velocity")
        normals = np.asarray(sd.face_normals, dtype=np.float64).reshape(3, -1)
        nf = normals.shape[1]
        flux = vel @ normals
        if cell_apertures is not None and nf:
            inc = abs(sps.csr_matrix(sd.cell_faces))  # faces x cells incidence
            cells_per_face = np.diff(inc.indptr)
            flux = flux * ((inc @ np.asarray(cell_apertures, dtype=np.float64)) / cells_per_face)
        return flux

    # ---- beyond the reference: the transport step on the device -------------------------
    def solve(self, sd, data: dict, accumulation=None, c_old=None, source=None, method: str = "bicgstab",
              rtol: float = 1e-12, maxit: int = 20000, x0=None, restart: int = 0, precond: str = "jacobi"):
        """Solve ``(diag(accumulation) + A) c = accumulation * c_old - b_ref + source``.  Returns (c, info).

        The matrix of an acyclic flow field is triangular up to a permutation; BiCGStab (the default) breaks down on
        it when the right-hand side sits in cells nothing flows back into -- injection into a field at rest, in any
        dimension.  ``method="gmres"`` solves those; ``advance`` switches by itself.

        ``precond="sweep"``: one substitution in flow order (``context(sd).sweep_info()``).  When the flux graph is
        acyclic it is exact -- the solve is one sweep and one residual check, ``info["iterations"] == 1``, whatever
        ``method`` says.  Where the flux has cycles (``stats()["sweep_core_cells"] > 0``) the cells of the cyclic core
        are treated by Jacobi against their upstream values and the sweep preconditions ``method``."""
        self._assemble(sd, data, accumulation, c_old, source)
        return self.context(sd).solve(method=method, rtol=rtol, maxit=maxit, x0=x0, restart=restart, precond=precond)

    def advance(self, sd, data: dict, c0, n_steps: int, accumulation, source=None, method: str = "bicgstab",
                rtol: float = 1e-12, maxit: int = 20000, raise_on_fail: bool = True, precond: str = "jacobi"):
        """``n_steps`` implicit Euler steps from ``c0`` with ``accumulation`` = porosity x volume / dt per cell, all
        on the device.  Returns (c_n, info); info["steps_done"] counts the converged steps.  A step whose BiCGStab solve
        breaks down (see ``solve``) is solved again with GMRES from the kept state; ``context(sd).stats()
        ["transport_gmres_retries"]`` counts them.

        ``precond="sweep"`` (default "jacobi"): every step is one substitution in flow order plus a residual check when
        the flux graph is acyclic (``stats()["sweep_direct_steps"]`` counts them); with a cyclic core the sweep
        preconditions ``method`` (see ``solve``).  The order is built once per flux."""
        self._assemble(sd, data, accumulation, None, source)
        return self.context(sd).transport_advance(c0, n_steps, method=method, rtol=rtol, maxit=maxit,
                                                  raise_on_fail=raise_on_fail, precond=precond)

    def advance_components(self, sd, data: dict, c0, n_steps: int, accumulation, bc_values=None, source=None,
                           method: str = "bicgstab", rtol: float = 1e-12, maxit: int = 20000,
                           raise_on_fail: bool = True, precond: str = "jacobi"):
        """``n_steps`` implicit Euler steps of k quantities carried by the one flux of the (one-component)
        discretization: solutes with different retardation, a tracer and a temperature.  ``c0``: (k, Nc).
        ``accumulation``: (Nc,) shared or (k, Nc).  ``bc_values``: None (the keyword's for every component), (Nf,) or
        (k, Nf).  ``source``: None, (Nc,) or (k, Nc).  Returns (c, info): c of shape (k, Nc), info["steps_done"] the
        steps completed by all components and the per-component lists "iterations", "rel_residual", "converged".

        ``precond="sweep"`` on an acyclic flux: every step is ONE substitution in flow order that carries all k
        components -- the matrix, the levels and the launches are those of a single component
        (``stats()["transport_multi_direct_steps"]``).  Any other case -- ``precond="jacobi"``, a cyclic core, a
        component whose residual check fails (``stats()["transport_multi_fallback_components"]``) -- steps the component
        as ``advance`` would.  Afterwards the handle holds no assembled transport system."""
        pd = data[PARAMETERS][self.keyword]
        c0 = np.asarray(c0, dtype=np.float64)
        nc, nf = sd.num_cells, sd.num_faces
        if c0.ndim != 2 or c0.shape[1] != nc:
            raise ValueError(f"c0 must have shape (k, {nc}), not {c0.shape}")
        k = c0.shape[0]
        if not 1 <= k <= 64:
            raise ValueError(f"the number of components must lie in 1 .. 64, not {k} (c0 has shape {c0.shape})")

        if accumulation is None:
            raise ValueError("accumulation is required")
        acc = per_component("accumulation", accumulation, k, nc)
        bv = per_component("bc_values", pd["bc_values"] if bc_values is None else bc_values, k, nf)
        src = None if source is None else per_component("source", source, k, nc)
        with _argument_errors():
            return self.context(sd).transport_advance_multi(c0, n_steps, acc, bv, q=self._flux(sd, pd), source=src,
                                                            method=method, rtol=rtol, maxit=maxit,
                                                            raise_on_fail=raise_on_fail, precond=precond)

    def adjoint_components(self, sd, data: dict, n_steps: int, accumulation, loads, obs_cells=None, states=None,
                           bc_values=None, want=("c0", "source", "bc_values"), rtol: float = 1e-12, maxit: int = 500,
                           raise_on_fail: bool = True):
        """The adjoint of ``advance_components``: the gradients of
        ``J = sum_{n=1..N} sum_a <loads[n-1, a], c_a^n[obs_cells]>`` through ``n_steps`` = N forward steps, for the
        cost of about one more run -- what a calibration of porosity, retardation, inflow concentrations, sources or
        the flux itself against breakthrough curves needs.  Per step, backwards in time, all k components are ONE
        transposed substitution in reverse flow order (``S_a^T lambda_a^n = g_a^n + acc_a o lambda_a^{n+1}``): the
        levels and the launches are those of the forward sweep.

        ``accumulation``: (Nc,) or (k, Nc) with k taken from ``loads``; ``loads``: (N, k, n_obs), dJ/dc^n on the
        observation cells; ``obs_cells``: n_obs cell indices without repeats, None = every cell; ``bc_values``: None
        (the keyword's), (Nf,) or (k, Nf); ``states``: (N + 1, k, Nc), c^0 .. c^N of the forward run, or None.
        ``want`` names the gradients:

        - ``"c0"`` (k, Nc): ``acc_a o lambda_a^1``;  ``"source"`` (k, Nc): ``sum_n lambda_a^n``;
        - ``"bc_values"`` (k, Nf): non-zero on Neumann faces and on Dirichlet inflow faces only;
        - ``"accumulation"`` (k, Nc): ``sum_n lambda_a^n o (c_a^{n-1} - c_a^n)`` -- needs ``states``;
        - ``"flux"`` (Nf,): ``-sum_n sum_a (lambda_a^n[p] - lambda_a^n[m]) cup_a^n`` with p / m the cells of
          ``cell_faces`` sign +1 / -1 and ``cup`` the upwind value at the face -- needs ``states``.  It is the
          derivative at a FIXED upstream side: valid wherever no ``q_f`` is exactly zero (a face whose flux changes sign
          has a kink there), zero on Neumann faces, whose flux is data.  The chain on to permeability, the flow
          boundary values and the flow source is ``Mpfa.adjoint_flow`` / ``Tpfa.adjoint_flow`` with this array as
          ``grad_flux``.

        The cells of a cyclic core are iterated by Jacobi on their transposed rows, at most ``maxit`` times per step.
        Returns (grads, info): a dict by the names in ``want``, and info["steps_done"], "converged" and the
        per-component lists "iterations" (1, or the core iterations of the last step) and "rel_residual".  Afterwards
        the handle holds no assembled transport system; the flow order stays."""
        pd = data[PARAMETERS][self.keyword]
        nc, nf = sd.num_cells, sd.num_faces
        loads = np.asarray(loads, dtype=np.float64)
        if loads.ndim != 3 or loads.shape[0] != int(n_steps):
            raise ValueError(f"loads must have shape ({int(n_steps)}, k, n_obs), not {loads.shape}")
        k = loads.shape[1]
        if not 1 <= k <= 64:
            raise ValueError(f"the number of components must lie in 1 .. 64, not {k} (loads has shape {loads.shape})")

        if accumulation is None:
            raise ValueError("accumulation is required")
        acc = per_component("accumulation", accumulation, k, nc)
        bv = per_component("bc_values", pd["bc_values"] if bc_values is None else bc_values, k, nf)
        with _argument_errors():
            return self.context(sd).transport_adjoint_multi(n_steps, acc, bv, loads, obs_cells=obs_cells, states=states,
                                                            q=self._flux(sd, pd), want=want, rtol=rtol, maxit=maxit,
                                                            raise_on_fail=raise_on_fail)

    def advance_saturation(self, sd, data: dict, s0, n_steps: int, accumulation, flux_function, source=None, sink=None,
                           rtol: float = 1e-12, maxit: int = 500, raise_on_fail: bool = True):
        """``n_steps`` implicit upwind steps of a saturation that moves with ``q f(s)`` -- the transport step of
        immiscible two-phase flow without gravity and capillary pressure:
        ``acc (s - s_old) + (A_ii + sink) f(s_i) + sum_j A_ij f(s_j) + b_ref = source``.  ``flux_function``: ``"linear"``,
        a ``CoreyFractionalFlow`` or a ``TabulatedFractionalFlow``.  A Dirichlet inflow value of the keyword's
        ``bc_values`` is a saturation, a Neumann value a flux of the transported phase.  ``accumulation`` (Nc, positive)
        = porosity x volume / dt; ``sink`` (Nc, >= 0) a production rate that takes fluid at the cell's own ``f(s)``.

        In flow order the step is one scalar monotone root-finding per cell, exact given its upstream cells: no
        Jacobian, no Krylov loop, no damping.  The cells of a cyclic core (``stats()["sweep_core_cells"]``) are iterated
        by nonlinear Jacobi, at most ``maxit`` times per step.  Returns (s, info): info["steps_done"] counts the accepted
        steps, "iterations" is 1 (or the core iterations of the last step), "rel_residual" the measured
        ``||F(s)|| / ||rhs||``.  A step that would leave [0, 1] raises ``ValueError`` naming the step and the cell; the
        error carries ``state``, the saturation before that step, and ``info``."""
        pd = data[PARAMETERS][self.keyword]
        kind, params = _flux_function(flux_function)
        if accumulation is None:
            raise ValueError("accumulation is required")
        with _argument_errors(with_state=True):
            s, info = self.context(sd).transport_advance_nl(
                s0, n_steps, accumulation, np.asarray(pd["bc_values"], dtype=float), kind, params, q=self._flux(sd, pd),
                source=source, sink=sink, rtol=rtol, maxit=maxit, raise_on_fail=raise_on_fail)
        return s, info

    def advance_saturation_components(self, sd, data: dict, s0, c0, n_steps: int, accumulation, flux_function,
                                      c_bc_values=None, sorption=None, source=None, sink=None, c_source=None,
                                      rtol: float = 1e-12, maxit: int = 500, raise_on_fail: bool = True):
        """``advance_saturation`` with k components carried by the transported phase -- salinity, a polymer, a tracer
        that marks injected water, the water's heat content.  ``c0``: (k, Nc), the amount per unit volume of the phase.
        With ``phi = f(s)`` of the step, component a solves
        ``(acc s + sorption_a) c_a + (A + diag(sink)) (phi c_a) = (acc s_old + sorption_a) c_old_a - b_ref_a + c_source_a``.
        ``c_bc_values``: None (zeros), (Nf,) or (k, Nf) -- on a Dirichlet inflow face the concentration in the entering
        phase (the saturation there is still the keyword's ``bc_values``), on a Neumann face the component's flux.
        ``sorption`` (>= 0, a capacity that does not scale with ``s``) and ``c_source`` (a mass rate): None, (Nc,) or
        (k, Nc).  The sink takes the component at ``sink f(s) c``.

        In flow order a component is one division per cell once the cell's saturation is known: the components ride in
        the launches of the saturation (``stats()["sweep_launches"]`` is that of ``advance_saturation``), and ``s`` is
        bit for bit what ``advance_saturation`` returns.  The cells of a cyclic core iterate ``s`` and ``c`` jointly.
        Returns (s, c, info); a step is accepted only if the saturation and every component pass the residual check
        (``info["c_rel_residual"]``), there is no per-component fallback.  Errors as ``advance_saturation``; the
        ``ValueError`` of a refused step carries ``state = (s, c)`` before that step, and ``info``."""
        pd = data[PARAMETERS][self.keyword]
        kind, params = _flux_function(flux_function)
        if accumulation is None:
            raise ValueError("accumulation is required")
        c0 = np.asarray(c0, dtype=np.float64)
        nc, nf = sd.num_cells, sd.num_faces
        if c0.ndim != 2 or c0.shape[1] != nc:
            raise ValueError(f"c0 must have shape (k, {nc}), not {c0.shape}")
        k = c0.shape[0]
        if not 1 <= k <= 64:
            raise ValueError(f"the number of components must lie in 1 .. 64, not {k} (c0 has shape {c0.shape})")

        cbv = np.zeros((k, nf)) if c_bc_values is None else per_component("c_bc_values", c_bc_values, k, nf)
        ads = None if sorption is None else per_component("sorption", sorption, k, nc)
        csrc = None if c_source is None else per_component("c_source", c_source, k, nc)
        with _argument_errors(with_state=True):
            return self.context(sd).transport_advance_nl_multi(
                s0, c0, n_steps, accumulation, np.asarray(pd["bc_values"], dtype=float), cbv, kind, params,
                q=self._flux(sd, pd), sorption=ads, source=source, sink=sink, c_source=csrc, rtol=rtol, maxit=maxit,
                raise_on_fail=raise_on_fail)

    def advance_reactive_components(self, sd, data: dict, c0, n_steps: int, accumulation, rate_matrix, rate_weight=None,
                                    mobility=None, bc_values=None, source=None, rtol: float = 1e-12, maxit: int = 500,
                                    raise_on_fail: bool = True):
        """``n_steps`` implicit Euler steps of k (1 .. 8) COUPLED components on the one flux of the (one-component)
        discretization -- a radionuclide decay chain, reversible first-order kinetics, kinetic sorption or
        mobile-immobile exchange, biodegradation with a yield:
        ``acc_a (c_a - c_old_a) + w_a (A c_a + b_ref_a) + rate_weight * (K c)_a = source_a``.
        ``rate_matrix`` K (k, k) is the rate matrix of ``dc/dt = -K c``, shared by all cells; ``rate_weight`` (Nc, >= 0,
        None = 1) weighs the reaction term per cell (pore volume x dt, a reactive zone); ``mobility`` w (k, >= 0,
        None = 1): 0 is an immobile component that sees no flux and no boundary (its boundary values are not read).
        ``c0``: (k, Nc); ``accumulation`` (positive), ``bc_values`` and ``source`` broadcast as in ``advance_components``.

        K must have a non-negative diagonal, non-positive off-diagonal entries and no negative column sum (no mass
        created; rounding of the sum is allowed for) -- ``ValueError`` otherwise.  Every cell's k x k block then is a
        column-diagonally-dominant M-matrix, solved without pivoting; non-negative data stay non-negative.

        In flow order a cell is one k x k solve once its upstream cells are known: the matrix, the levels and the
        launches are those of one component.  The cells of a cyclic core are iterated by block Jacobi, at most ``maxit``
        times per step.  Returns (c, info): info["steps_done"], "converged" and the per-component lists "iterations"
        (1, or the core iterations of the last step) and "rel_residual".  The error of a refused step carries
        ``state``, c before that step, and ``info``."""
        pd = data[PARAMETERS][self.keyword]
        c0 = np.asarray(c0, dtype=np.float64)
        nc, nf = sd.num_cells, sd.num_faces
        if c0.ndim != 2 or c0.shape[1] != nc:
            raise ValueError(f"c0 must have shape (k, {nc}), not {c0.shape}")
        k = c0.shape[0]
        if not 1 <= k <= 8:
            raise ValueError(f"the number of coupled components must lie in 1 .. 8, not {k} (c0 has shape {c0.shape})")

        if accumulation is None:
            raise ValueError("accumulation is required")
        acc = per_component("accumulation", accumulation, k, nc)
        bv = per_component("bc_values", pd["bc_values"] if bc_values is None else bc_values, k, nf)
        src = None if source is None else per_component("source", source, k, nc)
        with _argument_errors(with_state=True):
            return self.context(sd).transport_advance_react(c0, n_steps, acc, bv, rate_matrix, rate_weight=rate_weight,
                                                            mobility=mobility, q=self._flux(sd, pd), source=src,
                                                            rtol=rtol, maxit=maxit, raise_on_fail=raise_on_fail)

    def advance_sorbing_components(self, sd, data: dict, c0, n_steps: int, accumulation, isotherms, capacity=None,
                                   bc_values=None, source=None, rtol: float = 1e-12, maxit: int = 500,
                                   raise_on_fail: bool = True):
        """``n_steps`` implicit Euler steps of k (1 .. 64) concentrations ``c >= 0`` in equilibrium with a sorbed amount
        on a NONLINEAR isotherm, on the one flux of the (one-component) discretization -- Freundlich or Langmuir
        retardation: concentration-dependent retardation, self-sharpening fronts, tailing:
        ``acc_a (c_a - c_old_a) + capacity_a (S_a(c_a) - S_a(c_old_a)) + A c_a + b_ref_a = source_a``.
        ``isotherms``: a ``LinearIsotherm``, ``FreundlichIsotherm`` or ``LangmuirIsotherm`` for all components, or a
        list of k.  ``accumulation`` (positive) = porosity x volume / dt; ``capacity`` (>= 0, None = no sorption) = bulk
        density x volume / dt, with whatever scales the isotherm per cell.  ``c0``: (k, Nc), non-negative;
        ``accumulation``, ``capacity``, ``bc_values`` and ``source`` broadcast as in ``advance_components``, which
        remains the call for signed quantities.

        In flow order the step is one scalar monotone root-finding per cell and component, exact given its upstream
        cells: no Jacobian, no Krylov loop, no damping; the matrix, the levels and the launches are those of one
        component.  A linear isotherm is folded into the accumulation and is the division of ``advance_components``.
        The cells of a cyclic core are iterated by nonlinear Jacobi, at most ``maxit`` times per step.  Returns
        (c, info): info["steps_done"], "converged", the per-component lists "iterations" (1, or the core iterations of
        the last step) and "rel_residual", and "sorbed" (k, Nc), ``S_a(c_a)`` of the returned state.  A step in which a
        cell has no root ``c >= 0`` (a sink that takes more than the cell holds) raises ``ValueError`` naming the step,
        the cell and the component; the error of a refused step carries ``state``, c before that step, and ``info``."""
        pd = data[PARAMETERS][self.keyword]
        c0 = np.asarray(c0, dtype=np.float64)
        nc, nf = sd.num_cells, sd.num_faces
        if c0.ndim != 2 or c0.shape[1] != nc:
            raise ValueError(f"c0 must have shape (k, {nc}), not {c0.shape}")
        k = c0.shape[0]
        if not 1 <= k <= 64:
            raise ValueError(f"the number of components must lie in 1 .. 64, not {k} (c0 has shape {c0.shape})")
        iso = list(isotherms) if isinstance(isotherms, (list, tuple)) else [isotherms] * k
        if len(iso) != k:
            raise ValueError(f"isotherms must be one isotherm or a list of {k}, not {len(iso)}")
        for a, one in enumerate(iso):
            if not isinstance(one, (LinearIsotherm, FreundlichIsotherm, LangmuirIsotherm)):
                raise ValueError(f"isotherms[{a}] must be a LinearIsotherm, a FreundlichIsotherm or a LangmuirIsotherm, "
                                 f"not {one!r}")
        if accumulation is None:
            raise ValueError("accumulation is required")
        acc = per_component("accumulation", accumulation, k, nc)
        cap = None if capacity is None else per_component("capacity", capacity, k, nc)
        bv = per_component("bc_values", pd["bc_values"] if bc_values is None else bc_values, k, nf)
        src = None if source is None else per_component("source", source, k, nc)
        with _argument_errors(with_state=True):
            return self.context(sd).transport_advance_sorb(
                c0, n_steps, acc, bv, [one.kind for one in iso], np.array([one.params() for one in iso]), capacity=cap,
                q=self._flux(sd, pd), source=src, rtol=rtol, maxit=maxit, raise_on_fail=raise_on_fail)

    def adjoint_reactive_components(self, sd, data: dict, n_steps: int, accumulation, rate_matrix, loads,
                                    rate_weight=None, mobility=None, obs_cells=None, states=None, bc_values=None,
                                    want=("c0", "source", "bc_values"), rtol: float = 1e-12, maxit: int = 500,
                                    raise_on_fail: bool = True):
        """The adjoint of ``advance_reactive_components``: the gradients of
        ``J = sum_{n=1..N} sum_a <loads[n-1, a], c_a^n[obs_cells]>`` through ``n_steps`` = N reactive steps, for the
        cost of about one more run -- what a calibration of decay constants, exchange rates, the extent of a reactive
        zone or inflow concentrations against breakthrough curves needs.  The step is linear in c, so the adjoint is
        exact.  Per step, backwards in time, all k components are ONE transposed sweep in reverse flow order in which
        every cell is one k x k solve with the transposed block (``M^T lambda^n = g^n + acc o lambda^{n+1}``): the levels
        and the launches are those of the forward sweep.

        ``accumulation``, ``rate_matrix``, ``rate_weight``, ``mobility`` and ``bc_values`` as in
        ``advance_reactive_components`` (k is taken from ``loads``; the boundary values of an immobile component are
        not read); ``loads``, ``obs_cells`` and ``states`` as in ``adjoint_components``.  ``want`` names the gradients:

        - ``"c0"``, ``"source"``, ``"accumulation"`` (k, Nc) and ``"flux"`` (Nf,) as in ``adjoint_components``, the
          flux term of component a weighted by its mobility ``w_a`` (an immobile component is skipped);
        - ``"bc_values"`` (k, Nf): ``-w_a sum_n B^T lambda_a^n``, all zero for an immobile component;
        - ``"rate_matrix"`` (k, k): ``-sum_n sum_i rate_weight_i lambda_ia^n c_ib^n``.  It is the plain partial
          derivative with respect to EVERY entry of K, structural zeros included, without regard to the sign and
          column-sum conditions: chain it to your own rate parameters (a decay constant l of the chain a -> b enters as
          ``K_aa = l, K_ba = -l``, so ``dJ/dl = g[a, a] - g[b, a]``);
        - ``"rate_weight"`` (Nc,): ``-sum_n sum_a lambda_ia^n (K c_i^n)_a``.

        ``"accumulation"``, ``"flux"``, ``"rate_matrix"`` and ``"rate_weight"`` need ``states``, which are not checked
        for finiteness.  The gradient with respect to the mobility is not offered.  The cells of a cyclic core are
        iterated by block Jacobi, at most ``maxit`` times per step.  Returns (grads, info) as ``adjoint_components``.
        Afterwards the handle holds no assembled transport system; the flow order stays."""
        pd = data[PARAMETERS][self.keyword]
        nc, nf = sd.num_cells, sd.num_faces
        loads = np.asarray(loads, dtype=np.float64)
        if loads.ndim != 3 or loads.shape[0] != int(n_steps):
            raise ValueError(f"loads must have shape ({int(n_steps)}, k, n_obs), not {loads.shape}")
        k = loads.shape[1]
        if not 1 <= k <= 8:
            raise ValueError(f"the number of coupled components must lie in 1 .. 8, not {k} (loads has shape {loads.shape})")

        if accumulation is None:
            raise ValueError("accumulation is required")
        acc = per_component("accumulation", accumulation, k, nc)
        bv = per_component("bc_values", pd["bc_values"] if bc_values is None else bc_values, k, nf)
        with _argument_errors():
            return self.context(sd).transport_adjoint_react(n_steps, acc, bv, rate_matrix, loads, rate_weight=rate_weight,
                                                            mobility=mobility, obs_cells=obs_cells, states=states,
                                                            q=self._flux(sd, pd), want=want, rtol=rtol, maxit=maxit,
                                                            raise_on_fail=raise_on_fail)

    def adjoint_saturation(self, sd, data: dict, n_steps: int, accumulation, flux_function, loads, states, sink=None,
                           obs_cells=None, want=("s0", "source", "bc_values"), rtol: float = 1e-12, maxit: int = 500,
                           raise_on_fail: bool = True):
        """The adjoint of ``advance_saturation``: the gradients of ``J = sum_{n=1..N} <loads[n-1], s^n[obs_cells]>``
        through ``n_steps`` = N saturation steps, for the cost of about one more run -- what a match of water-cut or
        saturation observations by Corey exponents, the viscosity ratio, residual saturations, porosity, well rates or
        the flux needs, without finite differences over whole runs.  The step is linearised about the forward states:
        per step, backwards in time, ``(diag(acc) + diag(f'(s^n)) M^T) lambda^n = loads^n + acc o lambda^{n+1}`` is ONE
        transposed sweep in reverse flow order, a division per cell; the levels and the launches are those of the
        forward sweep.

        ``accumulation``, ``flux_function`` and ``sink`` as in ``advance_saturation`` (the source does not enter);
        ``loads``: (N, n_obs); ``obs_cells``: n_obs cell indices without repeats, or None (every cell, in order);
        ``states``: (N + 1, Nc), s^0 .. s^N of the forward run -- required, and not checked for range or finiteness.
        ``want`` names the gradients:

        - ``"s0"``, ``"source"``, ``"accumulation"`` (Nc,): ``acc o lambda^1``, ``sum_n lambda^n``,
          ``sum_n lambda^n o (s^{n-1} - s^n)``;
        - ``"sink"`` (Nc,): ``-sum_n lambda^n o f(s^n)``; with ``sink=None`` the derivative at sink = 0;
        - ``"bc_values"`` (Nf,): on a Neumann face the flux value's, on a Dirichlet inflow face the saturation's
          (``-sum_n (lambda_p - lambda_m) q_f f'(bv_f)``), zero on every other face;
        - ``"flux"`` (Nf,): ``-sum_n (lambda_p - lambda_m) f(s_upstream^n)`` (``f(bv_f)`` on a Dirichlet inflow face,
          zero on a Neumann face);
        - ``"flux_function"`` (6,): a ``CoreyFractionalFlow`` only (``ValueError`` otherwise), ordered as
          ``CoreyFractionalFlow.params``: s_wr, s_nr, n_w, n_n, mu_w, mu_n.  Gradients with respect to the values of a
          table are not offered.

        Every gradient is the derivative on a FIXED branch: of the interval of a table, of the side of a residual
        saturation, of the upstream side of every face.  J has kinks where a state sits on a table knot or on a
        residual saturation and where a ``q_f`` is exactly zero: there the gradient is a one-sided derivative, elsewhere
        the derivative.  The chain from ``"flux"`` to a permeability is ``Mpfa.adjoint_flow`` /
        ``Tpfa.adjoint_flow`` with that array as ``grad_flux``.

        The cells of a cyclic core are iterated by Jacobi on their transposed rows, at most ``maxit`` times per step.
        Returns (grads, info): info["steps_done"], "converged", "iterations" (1, or the core iterations of the last
        step) and "rel_residual" (the measured ``||r - J^T lambda|| / ||r||``).  A refused step leaves the gradients
        zero.  Afterwards the handle holds no assembled transport system; the flow order stays."""
        pd = data[PARAMETERS][self.keyword]
        kind, params = _flux_function(flux_function)
        if accumulation is None:
            raise ValueError("accumulation is required")
        with _argument_errors():
            return self.context(sd).transport_adjoint_nl(
                n_steps, accumulation, np.asarray(pd["bc_values"], dtype=float), kind, params, loads, states, sink=sink,
                obs_cells=obs_cells, q=self._flux(sd, pd), want=want, rtol=rtol, maxit=maxit, raise_on_fail=raise_on_fail)


    def adjoint_saturation_components(self, sd, data: dict, n_steps: int, accumulation, flux_function, s_states,
                                      c_states, s_loads=None, c_loads=None, c_bc_values=None, sorption=None, sink=None,
                                      obs_cells=None, want=("s0", "c0", "source", "c_source"), rtol: float = 1e-12,
                                      maxit: int = 500, raise_on_fail: bool = True):
        """The adjoint of ``advance_saturation_components``: the gradients of
        ``J = sum_{n=1..N} [<s_loads[n-1], s^n[obs_cells]> + sum_a <c_loads[n-1, a], c_a^n[obs_cells]>]`` through
        ``n_steps`` = N steps of the saturation with its k phase-carried components, for the cost of about one more
        run -- what a match of tracer, salinity or polymer breakthrough curves needs: there the concentrations depend
        on the saturation run and through it on the Corey parameters, porosity, well rates and the flux.  With the
        multipliers ``lambda`` (saturation) and ``mu_a`` (component a), ``e_a = acc s^n + sorption_a``, per step,
        backwards in time,
        ``(diag(e_a) + diag(f(s^n)) M^T) mu_a^n = c_loads_a^n + e_a o mu_a^{n+1}`` and
        ``(diag(acc) + diag(f'(s^n)) M^T) lambda^n = s_loads^n + acc o lambda^{n+1} - sum_a c_a^n o [acc o (mu_a^n -
        mu_a^{n+1}) + f'(s^n) o (M^T mu_a^n)]`` are ONE fused transposed sweep in reverse flow order, k + 1 divisions per
        cell; the levels and the launches are those of the forward sweep.

        ``accumulation``, ``flux_function``, ``c_bc_values``, ``sorption`` and ``sink`` as in
        ``advance_saturation_components`` (the sources do not enter; ``c_bc_values`` and ``sorption`` broadcast the same
        way).  ``s_states``: (N + 1, Nc) and ``c_states``: (N + 1, k, Nc), the forward run's s^0 .. s^N and c^0 .. c^N --
        both required, not checked for range or finiteness; k (1 .. 64) is taken from ``c_states``.  ``s_loads``:
        (N, n_obs), ``c_loads``: (N, k, n_obs); at least one is given, a missing one is zeros.  ``obs_cells``: n_obs
        cell indices without repeats, or None (every cell, in order).  ``want`` names the gradients:

        - ``"s0"`` (Nc,): ``acc o lambda^1 + sum_a acc o c_a^0 o mu_a^1``; ``"c0"`` (k, Nc): ``(acc s^0 + sorption_a) o mu_a^1``;
        - ``"source"`` (Nc,): ``sum_n lambda^n``; ``"c_source"`` (k, Nc): ``sum_n mu_a^n``;
        - ``"accumulation"`` (Nc,): ``-sum_n [lambda^n o (s^n - s^{n-1}) + sum_a mu_a^n o (s^n c_a^n - s^{n-1} c_a^{n-1})]``;
        - ``"sorption"`` (k, Nc): ``-sum_n mu_a^n o (c_a^n - c_a^{n-1})``; with ``sorption=None`` the derivative at zero;
        - ``"sink"`` (Nc,): ``-sum_n f(s^n) o (lambda^n + sum_a mu_a^n o c_a^n)``;
        - ``"bc_values"`` (Nf,): the saturation's boundary value -- a Neumann face as ``adjoint_saturation``, a Dirichlet
          inflow face ``-sum_n q_f f'(bv_f) [(lambda_p - lambda_m) + sum_a (mu_ap - mu_am) cbv_af]``;
        - ``"c_bc_values"`` (k, Nf): on a Neumann face the component flux's, on a Dirichlet inflow face
          ``-sum_n (mu_ap - mu_am) q_f f(bv_f)``, zero on every other face;
        - ``"flux"`` (Nf,): ``-sum_n [(lambda_p - lambda_m) f_up + sum_a (mu_ap - mu_am) f_up c_up,a]`` with the upstream
          cell's ``f(s^n)`` and ``c_a^n`` (``f(bv_f)`` and ``cbv_af`` on a Dirichlet inflow face, zero on a Neumann face);
        - ``"flux_function"`` (6,): a ``CoreyFractionalFlow`` only (``ValueError`` otherwise), ordered as
          ``CoreyFractionalFlow.params``.

        Every gradient is the derivative on a FIXED branch, as in ``adjoint_saturation``.  A dry row -- a cell and
        component with ``acc s^n + sorption_a + f(s^n) (outflow + sink) = 0``, where the forward step keeps ``c`` and
        does not determine it -- raises ``ValueError`` naming the step, the cell and the component; cells on a flat part
        of the curve (``f' = 0``) are fine.

        The cells of a cyclic core iterate ``mu`` and ``lambda`` jointly by Jacobi on their transposed rows, at most
        ``maxit`` times per step.  Returns (grads, info): info["steps_done"], "converged", "iterations" (1, or the core
        iterations of the last step), "rel_residual" (the saturation's) and "c_rel_residual" (per component).  A refused
        step leaves the gradients zero.  Afterwards the handle holds no assembled transport system; the flow order
        stays."""
        pd = data[PARAMETERS][self.keyword]
        kind, params = _flux_function(flux_function)
        if accumulation is None:
            raise ValueError("accumulation is required")
        if s_states is None or c_states is None:
            raise ValueError("s_states (s^0 .. s^N) and c_states (c^0 .. c^N) are required: the step is linearised "
                             "about them")
        nc, nf = sd.num_cells, sd.num_faces
        c_states = np.asarray(c_states, dtype=np.float64)
        if c_states.ndim != 3 or c_states.shape[0] != int(n_steps) + 1 or c_states.shape[2] != nc:
            raise ValueError(f"c_states must have shape ({int(n_steps) + 1}, k, {nc}), not {c_states.shape}")
        k = c_states.shape[1]
        if not 1 <= k <= 64:
            raise ValueError(f"the number of components must lie in 1 .. 64, not {k} (c_states has shape "
                             f"{c_states.shape})")

        cbv = np.zeros((k, nf)) if c_bc_values is None else per_component("c_bc_values", c_bc_values, k, nf)
        ads = None if sorption is None else per_component("sorption", sorption, k, nc)
        with _argument_errors():
            return self.context(sd).transport_adjoint_nl_multi(
                n_steps, accumulation, np.asarray(pd["bc_values"], dtype=float), cbv, kind, params, s_states, c_states,
                s_loads=s_loads, c_loads=c_loads, sorption=ads, sink=sink, obs_cells=obs_cells, q=self._flux(sd, pd),
                want=want, rtol=rtol, maxit=maxit, raise_on_fail=raise_on_fail)


def _flux_function(flux_function):
    """(kind, parameters) of the C ABI for what ``advance_saturation`` takes as ``flux_function``"""
    if isinstance(flux_function, str) and flux_function == "linear":
        return _lib.FLUXFN_LINEAR, ()
    if isinstance(flux_function, (CoreyFractionalFlow, TabulatedFractionalFlow)):
        return flux_function.kind, flux_function.params
    raise ValueError('flux_function must be "linear", a CoreyFractionalFlow or a TabulatedFractionalFlow')


def as_porepy_upwind(device: int = 0, library=None):
    """Subclass of the reference's ``pp.Upwind`` whose discretization and assembly run on the device; rebind with
    ``pp.Upwind = porepy_amd.as_porepy_upwind()`` before the model is built."""
    import porepy as pp  # the reference; absent on the GPU box

    _device, _library = device, library
    _Ref = pp.Upwind

    class HipUpwind(_Ref):  # type: ignore[misc]
        def __init__(self, keyword: str = "transport"):
            _Ref.__init__(self, keyword)
            self._hip = Upwind(keyword, _device, _library)

        def _sync_keys(self):
            h = self._hip
            h.keyword = self.keyword
            h.upwind_matrix_key = self.upwind_matrix_key
            h.bound_transport_dir_matrix_key = self.bound_transport_dir_matrix_key
            h.bound_transport_neu_matrix_key = self.bound_transport_neu_matrix_key
            h.flux_array_key = self.flux_array_key

        def discretize(self, sd, data):
            self._sync_keys()
            return self._hip.discretize(sd, data)

        def assemble_matrix_rhs(self, sd, data):
            self._sync_keys()
            if data[pp.PARAMETERS][self.keyword].get("num_components", 1) != 1 or sd.dim == 0:
                return _Ref.assemble_matrix_rhs(self, sd, data)
            return self._hip.assemble_matrix_rhs(sd, data)

    return HipUpwind
