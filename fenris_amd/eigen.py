"""The lowest eigenpairs of K phi = lambda M phi, matrix-free (fh_eigs_lowest, LOBPCG on the device).

MatrixFreeEigensolver finds natural frequencies and mode shapes of a clamped or free body, or -- with a nonlinear material and the
assembler's u -- the spectrum of the tangent of a prestressed state, without forming K or M.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from . import contact as _contact
from . import dirichlet as _dirichlet
from ._ffi import FenrisError
from .assembly import _is_torch


@dataclass
class EigenResult:
    """values ascending; vectors n x num_modes (numpy array, or a device tensor with device=True), M-orthonormal and zero on the Dirichlet
    dofs; residual_norms ||K x_i - theta_i M x_i||_2; iterations, map applications and restarts of the solve"""

    values: np.ndarray
    vectors: object
    residual_norms: np.ndarray
    iterations: int
    applications: int
    restarts: int
    preconditionings: int = 0


class EigenSolveError(FenrisError):
    """FH_EIG_MAX_ITERATIONS or FH_EIG_BREAKDOWN; `result` holds the pairs reached so far"""

    def __init__(self, code, message, result):
        super().__init__(code, message)
        self.result = result


class MatrixFreeEigensolver:
    """LOBPCG for the lowest modes of T(u) phi = lambda M phi on an element assembler (Laplace, LinearElastic, NeoHookean, StVK, StableNeoHookean): T(u) is
    MatrixFreeTangent's map at the assembler's u, M the mass of MatrixFreeShiftedTangent with this object's density.  Dirichlet nodes,
    density and shift belong to this object and are handed to the engine before every solve, so it may share an assembler with other
    matrix-free objects.  On a free body give with_shift(sigma), sigma > 0 of the order of the first elastic eigenvalue."""

    def __init__(self, element_assembler, density):
        self.element_assembler = element_assembler
        self.engine = element_assembler.engine
        self._nodes = None
        self._mg = None
        self.shift = 0.0
        self._rho = np.ascontiguousarray(np.atleast_1d(np.asarray(density, dtype=np.float64)).ravel()).copy()
        self.engine.set_mass_density(self._rho)   # (checks the count now)
        self.engine._mass_bound = self

    def with_dirichlet_nodes(self, nodes):
        self._nodes = None if nodes is None else _ffi.as_u64(nodes).copy()
        self._bind(force=True)
        return self

    def with_dirichlet_dofs(self, nodes, components):
        """single components of the listed nodes (MatrixFreeOperator.with_dirichlet_dofs): they leave the eigenproblem; calls accumulate; returns self"""
        return _dirichlet.with_dirichlet_dofs(self, nodes, components)

    def with_multigrid(self, mg):
        """a GeometricMultigrid over this assembler: solve then defaults to PRECOND_MULTIGRID; returns self"""
        self._mg = mg
        return self

    def with_shift(self, sigma):
        """the shift of the criterion and of the preconditioner's matrix sigma M + T(u) (>= 0); returns self"""
        self.shift = float(sigma)
        return self

    def _bind(self, force=False):
        # (the engine keeps the Dirichlet nodes and the density of the object that used it last, as for MatrixFreeShiftedTangent)
        if force or getattr(self.engine, "_mf_bound", None) is not self:
            self.engine.set_operator_dirichlet_nodes(self._nodes)
            self.engine._mf_bound = self
        if force or getattr(self.engine, "_mass_bound", None) is not self:
            self.engine.set_mass_density(self._rho)
            self.engine._mass_bound = self
        _contact.bind_obstacles(self, force)

    def with_element_expansion(self, theta):
        """the per-element expansion of the engine (Engine.set_element_expansion: a scalar, one stretch per element, None to clear it).  The
        field belongs to the engine, not to this object: every object on the same engine sees it until it is changed; returns self"""
        self.engine.set_element_expansion(theta)
        return self

    def with_obstacles(self, obstacles):
        """the rigid obstacles whose penalty term joins the stiffness: (T(u) + B(u)) phi = lambda M phi (None: none); returns self"""
        return _contact.with_obstacles(self, obstacles)

    def solve(self, num_modes, tol=1e-8, max_iter=0, preconditioner=None, guess=None, device=False):
        """The lowest num_modes pairs.  preconditioner None: PRECOND_MULTIGRID with a hierarchy (with_multigrid), else Jacobi.  guess: n x
        num_modes start vectors (numpy array or device tensor; columns are vectors), None: the library's own reproducible start block.
        device=True returns the vectors as a device tensor.  Raises EigenSolveError (with the partial EigenResult) when max_iter is
        exhausted or the basis breaks down."""
        import torch

        self._bind()
        if preconditioner is None:
            preconditioner = _ffi.PRECOND_MULTIGRID if self._mg is not None else _ffi.PRECOND_JACOBI
        if preconditioner == _ffi.PRECOND_MULTIGRID and self._mg is not None:
            self._mg._bind(self._nodes, self._rho if self.shift != 0.0 else None)
        m = int(num_modes)
        n = self.element_assembler.solution_dim() * self.engine.num_nodes()
        theta, resn, stats = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(4, dtype=np.uint64)
        lib = self.engine._lib
        mm = min(max(m, 0), _ffi.EIG_MAX_BLOCK)
        if device or _is_torch(guess):
            dev = f"cuda:{self.engine.device}"
            # column-major n x m: the transpose of a contiguous m x n tensor
            xt = torch.zeros((max(mm, 1), n), dtype=torch.float64, device=dev)
            if guess is not None:
                g = guess if _is_torch(guess) else torch.from_numpy(np.ascontiguousarray(guess, dtype=np.float64))
                if tuple(g.shape) != (n, m):
                    raise ValueError(f"guess must be {n} x {m}")
                xt[:m] = g.to(dev).T
            rc = lib.fh_eigs_lowest_dev(self.engine._h, m, self.shift, int(preconditioner), float(tol), int(max_iter), int(guess is not None),
                                        C.c_void_p(xt.data_ptr()), _ffi.fp(theta), _ffi.fp(resn), _ffi.up(stats))
            vectors = xt[:mm].T if device else xt[:mm].T.cpu().numpy()
        else:
            xh = np.zeros((max(mm, 1), n))
            if guess is not None:
                g = np.asarray(guess, dtype=np.float64)
                if g.shape != (n, m):
                    raise ValueError(f"guess must be {n} x {m}")
                xh[:m] = g.T
            rc = lib.fh_eigs_lowest(self.engine._h, m, self.shift, int(preconditioner), float(tol), int(max_iter), int(guess is not None),
                                    _ffi.fp(xh), _ffi.fp(theta), _ffi.fp(resn), _ffi.up(stats))
            vectors = xh[:mm].T
        res = EigenResult(theta[:mm].copy(), vectors, resn[:mm].copy(), int(stats[0]), int(stats[1]), int(stats[3]), int(stats[2]))
        if rc in (_ffi.FH_EIG_MAX_ITERATIONS, _ffi.FH_EIG_BREAKDOWN):
            raise EigenSolveError(rc, self.engine.last_error(), res)
        self.engine._check(rc)
        return res

    def profile(self):
        """fh_eigs_profile: seconds per phase of the last solve (maps, preconditioning, Gram, recombination, residuals, dense, other, total)"""
        out = np.zeros(8)
        self.engine._check(self.engine._lib.fh_eigs_profile(self.engine._h, _ffi.fp(out)))
        return out
