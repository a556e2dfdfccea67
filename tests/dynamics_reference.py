"""NumPy statement of the time integrators of fh_dynamics_* (include/fenris_hip.h), for tests/test_dynamics.py: central differences in
velocity-Verlet form with the row-sum lumped mass, Newmark(beta, gamma) and backward Euler with one Newton solve per step (the rule of
_np_newton in tests/test_newton.py), and the power iteration of fh_dynamics_stable_dt -- on the oracle's residual
(oracle.assemble_vector), energy (oracle.assemble_scalar), assembled tangent and assembled MASS_SCALAR / MASS_VECTOR matrix, with direct
solves on the free dofs (dense; `direct="sparse"` takes a sparse LU instead, which leaves rounding only as well, where a trajectory of
Newton solves on some thousand dofs would otherwise take minutes)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


class Problem:
    """M a + r(u) = lf_n f on one mesh.  groups: [(connectivity, weights, points), ...] -- one entry for a uniform table, one per rule for a
    rule-set table, the active elements only under an element mask; rho: one density, or one array of per-element densities per group."""

    def __init__(self, oracle, okind, oop, vertices, groups, params=None, rho=1.0, dirichlet=(), f=None, load_factor=None, direct="dense"):
        self.o, self.okind, self.oop, self.vertices, self.groups, self.params = oracle, okind, oop, np.asarray(vertices), groups, params
        self.d = self.vertices.shape[1]
        self.s = 1 if oop == oracle.LAPLACE else self.d
        self.N = len(self.vertices)
        self.n = self.s * self.N
        self.rho = rho
        self.free = np.ones(self.n, dtype=bool)
        for k in range(self.s):
            self.free[self.s * np.asarray(dirichlet, dtype=np.int64) + k] = False
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor = None if load_factor is None else np.asarray(load_factor, dtype=np.float64)
        self.direct = direct
        self._mass = None

    def lf(self, n):
        return 1.0 if self.load_factor is None else float(self.load_factor[min(n, len(self.load_factor) - 1)])

    def _asm(self, g, u):
        conn, w, p = self.groups[g]
        return self.o.ElementAssembler(self.okind, self.oop, self.vertices, conn, w, p, params=self.params, u=u)

    def residual(self, u):
        r = np.zeros(self.n)
        for g in range(len(self.groups)):
            st, _, rg = self.o.assemble_vector(self._asm(g, u))
            assert st == 0
            r += rg
        return r

    def energy(self, u):
        tot = 0.0
        for g in range(len(self.groups)):
            st, _, e = self.o.assemble_scalar(self._asm(g, u))
            if st != 0:
                return float("nan")
            tot += e
        return tot

    def _csr(self, asm):
        st, _, ro, ci, vals = self.o.assemble(asm)
        assert st == 0
        return sp.csr_matrix((vals, ci.astype(np.int64), ro.astype(np.int64)), shape=(self.n, self.n))

    def tangent(self, u):
        K = self._csr(self._asm(0, u))
        for g in range(1, len(self.groups)):
            K = K + self._csr(self._asm(g, u))
        return K.tocsr()

    def mass(self):
        if self._mass is None:
            mop = self.o.MASS_SCALAR if self.s == 1 else self.o.MASS_VECTOR
            M = None
            for g, (conn, w, p) in enumerate(self.groups):
                if np.ndim(self.rho) == 0:
                    a = self.o.ElementAssembler(self.okind, mop, self.vertices, conn, w, p, params=[float(self.rho), 0.0])
                else:
                    re = np.asarray(self.rho[g], dtype=np.float64)
                    rp = np.zeros((len(re), len(w), 2))
                    rp[:, :, 0] = re[:, None]
                    a = self.o.ElementAssembler(self.okind, mop, self.vertices, conn, w, p, elem_to_rule=np.arange(len(re), dtype=np.uint64),
                                                rule_params=rp)
                Mg = self._csr(a)
                M = Mg if M is None else M + Mg
            self._mass = M.tocsr()
        return self._mass

    def lumped(self):
        return np.asarray(self.mass() @ np.ones(self.n)).reshape(-1)

    def solve_free(self, A, b):
        """x with A_ff x_f = b_f and x = 0 on the Dirichlet dofs, by a direct solve"""
        fr = self.free
        x = np.zeros(self.n)
        Aff = A[fr][:, fr]
        if self.direct == "dense":
            x[fr] = np.linalg.solve(Aff.toarray() if sp.issparse(Aff) else Aff, b[fr])
        else:
            x[fr] = spla.splu(sp.csc_matrix(Aff)).solve(b[fr])
        return x


def splitmix_column0(n):
    """X(dof, 0) of fh_eigs_lowest's fill: (splitmix64(dof) >> 11) 2^-52 - 1"""
    z = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def _record(prob, rows, ke, u, step, dt):
    rows.append([ke, prob.energy(u), prob.lf(step) * float(prob.f @ u), step * dt])


def _is_record(j, steps, record_every):
    return j + 1 == steps or (record_every and (j + 1) % record_every == 0)


def central_difference(prob, u0, v0, dt, steps, record_every=0, start=0):
    """(u, v, a, records[k][4]) after `steps` steps from step index `start`"""
    fr = prob.free
    m = prob.lumped()
    assert (m[fr] > 0).all()
    u = np.array(u0, dtype=np.float64)
    v = np.where(fr, v0, 0.0)
    a = np.zeros(prob.n)
    a[fr] = (prob.lf(start) * prob.f - prob.residual(u))[fr] / m[fr]
    rows = []
    for j in range(steps):
        vh = v + 0.5 * dt * a
        u = np.where(fr, u + dt * vh, u)
        a = np.zeros(prob.n)
        a[fr] = (prob.lf(start + j + 1) * prob.f - prob.residual(u))[fr] / m[fr]
        v = np.where(fr, vh + 0.5 * dt * a, 0.0)
        if _is_record(j, steps, record_every):
            _record(prob, rows, 0.5 * float(np.sum(m[fr] * v[fr] ** 2)), u, start + j + 1, dt)
    return u, v, a, np.array(rows)


def newton(prob, F, J, u, tol, backtracking=True, max_it=60):
    """newton_line_search with the backtracking rule of _np_newton (tests/test_newton.py): (status, u, iterations)"""
    Fu = F(u)
    it = 0
    while True:
        fn = np.linalg.norm(Fu)
        if not np.isfinite(fn):
            return "nonfinite", u, it
        if fn <= tol:
            return "ok", u, it
        if it == max_it:
            return "maxit", u, it
        step = -prob.solve_free(J(u), Fu)
        if not backtracking:
            u = u + step
            Fu = F(u)
        else:
            g0, a_prev, a = 0.5 * fn * fn, 0.0, 1.0
            while True:
                u = u + (a - a_prev) * step
                Fu = F(u)
                if 0.5 * np.dot(Fu, Fu) <= (1.0 - 1e-4 * a) * g0:
                    break
                if a < 1e-6:
                    return "line_search", u, it
                a_prev, a = a, {1.0: 0.75, 0.75: 0.5, 0.5: 0.25}.get(a, 0.25 * a)
        it += 1


def implicit(prob, scheme, u0, v0, dt, steps, record_every=0, beta=0.25, gamma=0.5, tol=1e-8, backtracking=True, max_it=60, start=0):
    """Newmark(beta, gamma) (scheme "newmark") or backward Euler ("euler"): (status, u, v, a, records, steps_done, Newton iterations)"""
    fr = prob.free
    M = prob.mass()
    euler = scheme == "euler"
    nb = 1.0 if euler else beta
    u = np.array(u0, dtype=np.float64)
    v = np.where(fr, v0, 0.0)
    a = np.zeros(prob.n)
    if not euler:
        a = prob.solve_free(M, prob.lf(start) * prob.f - prob.residual(u))
    rows, iters = [], 0
    for j in range(steps):
        load = prob.lf(start + j + 1) * prob.f
        u_ref = np.where(fr, u + dt * v + (0.0 if euler else dt * dt * (0.5 - beta)) * a, u)

        def F(x):
            out = M @ (x - u_ref) + nb * dt * dt * (prob.residual(x) - load)
            out[~fr] = 0.0
            return out

        def J(x):
            return (M + nb * dt * dt * prob.tangent(x)).tocsr()

        status, un, it = newton(prob, F, J, u_ref.copy(), tol, backtracking, max_it)
        iters += it
        if status != "ok":
            return status, u, v, a, np.array(rows), j, iters
        if euler:
            vn = np.where(fr, (un - u) / dt, 0.0)
            a = np.where(fr, (vn - v) / dt, 0.0)
            v = vn
        else:
            an = np.where(fr, (un - u_ref) / (beta * dt * dt), 0.0)
            v = np.where(fr, v + dt * ((1.0 - gamma) * a + gamma * an), 0.0)
            a = an
        u = un
        if _is_record(j, steps, record_every):
            _record(prob, rows, 0.5 * float(v @ (M @ v)), u, start + j + 1, dt)
    return "ok", u, v, a, np.array(rows), steps, iters


def power_iteration(prob, u, iterations):
    """omega_max^2 as fh_dynamics_stable_dt forms it: the last Rayleigh quotient of x <- m^-1 T(u) x on the free dofs, m-normalised"""
    fr = prob.free
    m = prob.lumped()
    K = prob.tangent(u)
    x = np.where(fr, splitmix_column0(prob.n), 0.0)
    x /= np.sqrt(np.sum(m[fr] * x[fr] ** 2))
    rq = 0.0
    for _ in range(iterations):
        y = np.asarray(K @ x).reshape(-1)
        rq = float(x[fr] @ y[fr])
        x = np.zeros(prob.n)
        x[fr] = y[fr] / m[fr]
        x /= np.sqrt(np.sum(m[fr] * x[fr] ** 2))
    return rq


def dense_pencil(prob, u, lumped):
    """eigenvalues (ascending) and vectors of K phi = lambda B phi on the free dofs, B = diag m or the consistent M; vectors on all dofs"""
    import scipy.linalg as sl

    fr = prob.free
    K = prob.tangent(u)[fr][:, fr].toarray()
    B = np.diag(prob.lumped()[fr]) if lumped else prob.mass()[fr][:, fr].toarray()
    w, V = sl.eigh(0.5 * (K + K.T), 0.5 * (B + B.T))
    full = np.zeros((prob.n, V.shape[1]))
    full[fr] = V
    return w, full


def closed_form(scheme, omega, dt, n):
    """the factor c_n of u_n = c_n phi for u_0 = phi, v_0 = 0, f = 0 on one eigenmode of the scheme's pencil"""
    x = omega * dt
    if scheme == "central":
        return np.cos(n * 2.0 * np.arcsin(0.5 * x))
    if scheme == "newmark":
        return np.cos(n * 2.0 * np.arctan(0.5 * x))
    return (1.0 + x * x) ** (-0.5 * n) * np.cos(n * np.arctan(x))
