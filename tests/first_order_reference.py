"""NumPy statement of the first-order integrators of fh_first_order_create (include/fenris_hip.h), for tests/test_first_order.py:
M du/dt + r(u) = lf_n f by Runge-Kutta-Legendre super-steps with the row-sum lumped mass (one stage: forward Euler) and by the theta
method with the consistent mass (one Newton solve per step), on the Problem, the Newton rule and the direct solves of
tests/dynamics_reference.py."""
import numpy as np
from numpy.polynomial import legendre

from dynamics_reference import Problem, dense_pencil, newton, power_iteration  # noqa: F401  (the tests take them from here)


def _is_record(j, steps, record_every):
    return j + 1 == steps or (record_every and (j + 1) % record_every == 0)


def _record(prob, rows, norm, u, step, dt):
    rows.append([norm, prob.energy(u), prob.lf(step) * float(prob.f @ u), step * dt])


def lumped_rate(prob, m, y, n):
    """L(y) = (lf_n f - r(y)) / m on the free dofs, zero on the others"""
    out = np.zeros(prob.n)
    fr = prob.free
    out[fr] = (prob.lf(n) * prob.f - prob.residual(y))[fr] / m[fr]
    return out


def rkl(prob, u0, dt, stages, steps, record_every=0, start=0):
    """(u, rate, records[k][4]) after `steps` Runge-Kutta-Legendre steps of `stages` stages from step index `start`; every stage of step n
    takes lf_n; column 0 of a record is 1/2 sum m u^2 over all dofs"""
    fr = prob.free
    m = prob.lumped()
    assert (m[fr] > 0).all()
    s = int(stages)
    w1 = 2.0 / (s * s + s)
    u = np.array(u0, dtype=np.float64)
    rows = []
    for j in range(steps):
        n = start + j
        prev, cur = u, np.where(fr, u + w1 * dt * lumped_rate(prob, m, u, n), u)
        for k in range(2, s + 1):
            mu, nu = (2.0 * k - 1.0) / k, (1.0 - k) / k
            prev, cur = cur, np.where(fr, mu * cur + nu * prev + mu * w1 * dt * lumped_rate(prob, m, cur, n), cur)
        u = cur
        if _is_record(j, steps, record_every):
            _record(prob, rows, 0.5 * float(np.sum(m * u * u)), u, n + 1, dt)
    return u, lumped_rate(prob, m, u, start + steps), np.array(rows)


def theta_method(prob, u0, dt, theta, steps, record_every=0, tol=1e-8, backtracking=True, max_it=60, start=0):
    """(status, u, rate, records, steps_done, Newton iterations): M (u_{n+1} - u_n) + theta dt (r(u_{n+1}) - g) = 0 with
    g = (lf_{n+1} + c lf_n) f - c r(u_n), c = (1 - theta) / theta, solved by Newton from u_n; column 0 of a record is 1/2 u^T M u; the rate
    solves M w = lf_n f - r(u_n) on the free dofs"""
    fr = prob.free
    M = prob.mass()
    c = (1.0 - theta) / theta
    u = np.array(u0, dtype=np.float64)
    rows, iters = [], 0

    def rate(x, n):
        return prob.solve_free(M, prob.lf(n) * prob.f - prob.residual(x))

    for j in range(steps):
        n = start + j
        g = (prob.lf(n + 1) + c * prob.lf(n)) * prob.f
        if c != 0.0:
            g = g - c * prob.residual(u)
        un = u

        def F(x):
            out = M @ (x - un) + theta * dt * (prob.residual(x) - g)
            out[~fr] = 0.0
            return out

        def J(x):
            return (M + theta * dt * prob.tangent(x)).tocsr()

        status, x, it = newton(prob, F, J, u.copy(), tol, backtracking, max_it)
        iters += it
        if status != "ok":
            return status, u, rate(u, n), np.array(rows), j, iters
        u = x
        if _is_record(j, steps, record_every):
            _record(prob, rows, 0.5 * float(u @ (M @ u)), u, n + 1, dt)
    return "ok", u, rate(u, start + steps), np.array(rows), steps, iters


def closed_form(scheme, lam, dt, n, stages=1, theta=1.0):
    """the factor c_n of u_n = c_n phi for u_0 = phi, f = 0 on one eigenmode (eigenvalue lam) of the scheme's pencil: "rkl": the Legendre
    polynomial P_s(1 - 2 lam dt / (s^2 + s))^n; "theta": ((1 - (1 - theta) lam dt) / (1 + theta lam dt))^n"""
    if scheme == "rkl":
        s = int(stages)
        coef = np.zeros(s + 1)
        coef[s] = 1.0
        return float(legendre.legval(1.0 - 2.0 * lam * dt / (s * s + s), coef)) ** n
    return ((1.0 - (1.0 - theta) * lam * dt) / (1.0 + theta * lam * dt)) ** n
