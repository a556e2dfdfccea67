"""NumPy statement of the Rayleigh-damped time integrators of fh_dynamics_set_damping (include/fenris_hip.h), for tests/test_damping.py:

    M a + C(u) v + r(u) = lf_n f,    C(u) = eta_m M + eta_k T(u)

on tests/dynamics_reference.Problem -- the oracle's residual, assembled tangent and assembled mass, direct solves on the free dofs.  The
equations are integrated UNFOLDED: the implicit schemes solve for u with a(u) and v(u) written out and C = eta_m M + eta_k T(u_n) frozen at
the start of the step, so agreement with the device proves the folding into the Newton arguments that the library uses.  The scalar
recurrences at the end are the closed forms of one eigenmode, written without reference to the vector code."""
import numpy as np

import dynamics_reference as dr


def stiffness(prob, u):
    """T(u) of C: the element tangent alone -- a problem with obstacles (contact_reference.ContactMixin) leaves their term out of C"""
    return prob._base_tangent(u) if hasattr(prob, "_base_tangent") else prob.tangent(u)


def _force(prob, u, w, step, eta_k):
    """F(u, w) = lf f - r(u) - eta_k T(u) w"""
    out = prob.lf(step) * prob.f - prob.residual(u)
    if eta_k != 0.0:
        out = out - eta_k * np.asarray(stiffness(prob, u) @ w).reshape(-1)
    return out


def central_difference(prob, u0, v0, dt, steps, eta_m, eta_k, record_every=0, start=0):
    """velocity-Verlet with the lumped mass: a_0 = F(u_0, v_0) / m - eta_m v_0 and per step  v_h = v + dt/2 a,  u += dt v_h,
    a = (F(u, v_h) / m - eta_m v_h) / (1 + eta_m dt/2),  v = v_h + dt/2 a.  Returns (u, v, a, records[k][4])"""
    fr = prob.free
    m = prob.lumped()
    assert (m[fr] > 0).all()
    u = np.array(u0, dtype=np.float64)
    v = np.where(fr, v0, 0.0)
    a = np.zeros(prob.n)
    a[fr] = _force(prob, u, v, start, eta_k)[fr] / m[fr] - eta_m * v[fr]
    rows = []
    for j in range(steps):
        vh = v + 0.5 * dt * a
        u = np.where(fr, u + dt * vh, u)
        a = np.zeros(prob.n)
        a[fr] = (_force(prob, u, vh, start + j + 1, eta_k)[fr] / m[fr] - eta_m * vh[fr]) / (1.0 + 0.5 * eta_m * dt)
        v = np.where(fr, vh + 0.5 * dt * a, 0.0)
        if dr._is_record(j, steps, record_every):
            dr._record(prob, rows, 0.5 * float(np.sum(m[fr] * v[fr] ** 2)), u, start + j + 1, dt)
    return u, v, a, np.array(rows)


def damping_matrix(prob, u, eta_m, eta_k):
    """C(u) = eta_m M + eta_k T(u), assembled"""
    return (eta_m * prob.mass() + eta_k * stiffness(prob, u)).tocsr()


def implicit(prob, scheme, u0, v0, dt, steps, eta_m, eta_k, record_every=0, beta=0.25, gamma=0.5, tol=1e-8, backtracking=True, max_it=60, start=0):
    """Newmark(beta, gamma) ("newmark") or backward Euler ("euler") on the unfolded equation, C frozen at u_n; the Newton residual is
    scaled by b = beta dt^2 (Euler: dt^2) like the undamped reference's, so one tolerance serves both.  Returns dr.implicit's tuple"""
    fr = prob.free
    M = prob.mass()
    euler = scheme == "euler"
    b = dt * dt * (1.0 if euler else beta)
    u = np.array(u0, dtype=np.float64)
    v = np.where(fr, v0, 0.0)
    a = np.zeros(prob.n)
    if not euler:
        a = prob.solve_free(M, prob.lf(start) * prob.f - prob.residual(u) - np.asarray(damping_matrix(prob, u, eta_m, eta_k) @ v).reshape(-1))
    rows, iters = [], 0
    for j in range(steps):
        load = prob.lf(start + j + 1) * prob.f
        Cn = damping_matrix(prob, u, eta_m, eta_k)
        u_n, v_n, a_n = u, v, a
        u_ref = np.where(fr, u_n + dt * v_n + (0.0 if euler else dt * dt * (0.5 - beta)) * a_n, u_n)

        def acc(x):
            return (x - u_ref) / b

        def vel(x):
            if euler:
                return np.where(fr, (x - u_n) / dt, 0.0)
            return np.where(fr, v_n + dt * ((1.0 - gamma) * a_n + gamma * acc(x)), 0.0)

        def F(x):
            out = b * (np.asarray(M @ acc(x)).reshape(-1) + np.asarray(Cn @ vel(x)).reshape(-1) + prob.residual(x) - load)
            out[~fr] = 0.0
            return out

        dv = (1.0 if euler else gamma) * dt   # b dv/dx

        def J(x):
            return (M + dv * Cn + b * prob.tangent(x)).tocsr()

        status, un, it = dr.newton(prob, F, J, u_ref.copy(), tol, backtracking, max_it)
        iters += it
        if status != "ok":
            return status, u, v, a, np.array(rows), j, iters
        vn = vel(un)
        a = np.where(fr, (vn - v_n) / dt, 0.0) if euler else np.where(fr, acc(un), 0.0)
        v, u = vn, un
        if dr._is_record(j, steps, record_every):
            dr._record(prob, rows, 0.5 * float(v @ (M @ v)), u, start + j + 1, dt)
    return "ok", u, v, a, np.array(rows), steps, iters


# ---- one eigenmode: q'' + c q' + omega^2 q = 0 with c = eta_m + eta_k omega^2, from q_0 = 1, q'_0 = 0
def explicit_step_matrix(omega, dt, eta_m, eta_k):
    """the 2 x 2 matrix that takes (u_n, w_{n-1/2}) to (u_{n+1}, w_{n+1/2}), w the half-step velocity, n >= 1"""
    D = 1.0 + 0.5 * eta_m * dt
    c = eta_m + eta_k * omega * omega
    ww, wu = 1.0 - dt * c / D, -dt * omega * omega / D
    return np.array([[1.0 + dt * wu, dt * ww], [wu, ww]])


def closed_form(scheme, omega, dt, n, eta_m, eta_k):
    """the factor c_n of u_n = c_n phi for u_0 = phi, v_0 = 0, f = 0 on one eigenmode of the scheme's pencil"""
    c = eta_m + eta_k * omega * omega
    k = omega * omega
    if scheme == "central":
        w = 0.5 * dt * (-k)            # w_{1/2} = v_0 + dt/2 a_0, a_0 = -omega^2 (exact start: no divisor)
        s = np.array([1.0 + dt * w, w])
        return float((np.linalg.matrix_power(explicit_step_matrix(omega, dt, eta_m, eta_k), n - 1) @ s)[0])
    u, v, a = 1.0, 0.0, -k
    for _ in range(n):
        if scheme == "newmark":
            beta, gamma = 0.25, 0.5
            ur = u + dt * v + dt * dt * (0.5 - beta) * a
            vp = v + dt * (1.0 - gamma) * a
            a = -(c * vp + k * ur) / (1.0 + c * gamma * dt + k * beta * dt * dt)
            u, v = ur + beta * dt * dt * a, vp + gamma * dt * a
        else:
            ur = u + dt * v
            un = (ur / (dt * dt) + c * u / dt) / (1.0 / (dt * dt) + c / dt + k)
            v, u = (un - u) / dt, un
    return u


def dt_crit(omega, eta_k):
    """(2 / omega)(sqrt(1 + xi^2) - xi), xi = eta_k omega / 2: fh_dynamics_stable_dt's expression, each operation rounded once"""
    xi = eta_k * omega / 2.0
    x2 = xi * xi
    return (2.0 / omega) * (np.sqrt(1.0 + x2) - xi)
