"""References for the VV10 (NLC) term, all restating one formula, the energy

    E_nlc = sum_i w_i rho_i [ beta + 1/2 sum_j w_j rho_j Phi_ij ]      (j = i included)
    Phi_ij = -3/2 / (g_ij g_ji (g_ij + g_ji)),  g_ij = omega0_i R_ij^2 + kappa_i
    omega0 = sqrt(C gamma^2 / rho^4 + (4 pi / 3) rho),  kappa = b (3/2) pi (9 pi)^(-1/6) rho^(1/6)
    beta = (3 / b^2)^(3/4) / 32,   points with rho <= rho_min left out.

(a) ``mp_energy`` writes it literally in mpmath; ``mp_gradient`` and ``mp_hessian`` differentiate
    it by central differences with RELATIVE steps 1e-12 (truncation ~1e-24 relative).  The energy
    is evaluated at 40 digits; inside the second differences the working precision is raised to
    60 digits, because a second difference divides the rounding of E by the product of two steps
    (1e-40 / 1e-24 would leave only 16 digits).
(b) ``np_energy_ao`` is the same formula in complex-safe NumPy on AO values and a (complex)
    density matrix, for the complex-step derivative at the AO level.
(c) ``hess_apply`` / ``response_ao`` restate the analytic second derivative in NumPy (the host
    counterpart of csrc/xt_vv10.hip; the product has none).  It is pinned by (a) and (b) in
    tests/test_vv10_host.py and is what the GPU tests compare the device against.
"""
import numpy as np

RHO_MIN = 1e-8


# ---------------------------------------------------------------- (a) mpmath
def mp_energy(coords, w, rho, gamma, b, C, active, dps=40):
    """E_nlc over the points listed in `active` (those above rho_min), mpmath at `dps` digits.
    rho and gamma may hold mpf values."""
    import mpmath as mp
    with mp.workdps(dps):
        b, C = mp.mpf(b), mp.mpf(C)
        beta = (3 / b ** 2) ** mp.mpf('0.75') / 32
        kpref = b * mp.mpf(3) / 2 * mp.pi * (9 * mp.pi) ** (-mp.mpf(1) / 6)
        om, ka, a = {}, {}, {}
        for i in active:
            r, g = mp.mpf(rho[i]), mp.mpf(gamma[i])
            om[i] = mp.sqrt(C * g ** 2 / r ** 4 + 4 * mp.pi / 3 * r)
            ka[i] = kpref * r ** (mp.mpf(1) / 6)
            a[i] = mp.mpf(float(w[i])) * r
        e = mp.mpf(0)
        for i in active:
            inner = mp.mpf(0)
            for j in active:
                R2 = sum((mp.mpf(float(coords[i][k])) - mp.mpf(float(coords[j][k]))) ** 2 for k in range(3))
                gij = om[i] * R2 + ka[i]
                gji = om[j] * R2 + ka[j]
                inner += a[j] * (-mp.mpf(3) / 2) / (gij * gji * (gij + gji))
            e += a[i] * (beta + inner / 2)
        return +e


def _mp_vars(rho, gamma, active):
    import mpmath as mp
    # the variables: rho of the active points, then gamma of the active points
    return [mp.mpf(float(rho[i])) for i in active] + [mp.mpf(float(gamma[i])) for i in active]


def _mp_eval(coords, w, b, C, active, p, n_all, dps):
    rho = [0] * n_all
    gamma = [0] * n_all
    for k, i in enumerate(active):
        rho[i], gamma[i] = p[k], p[len(active) + k]
    return mp_energy(coords, w, rho, gamma, b, C, active, dps)


def mp_gradient(coords, w, rho, gamma, b, C, rho_min=RHO_MIN, rel=1e-12, dps=60):
    """(dE/drho, dE/dgamma) over all points (zero at masked points), as mpf lists."""
    import mpmath as mp
    active = [i for i in range(len(rho)) if float(rho[i]) > rho_min]
    with mp.workdps(dps):
        p = _mp_vars(rho, gamma, active)
        n = len(active)
        out = [[mp.mpf(0)] * len(rho), [mp.mpf(0)] * len(rho)]
        for k in range(2 * n):
            h = abs(p[k]) * mp.mpf(rel)
            pp, pm = list(p), list(p)
            pp[k] += h
            pm[k] -= h
            d = (_mp_eval(coords, w, b, C, active, pp, len(rho), dps) -
                 _mp_eval(coords, w, b, C, active, pm, len(rho), dps)) / (2 * h)
            out[k // n][active[k % n]] = d
        return out


def mp_hessian(coords, w, rho, gamma, b, C, rho_min=RHO_MIN, rel=1e-12, dps=60):
    """The Hessian of E over (rho_active, gamma_active) as an mpmath matrix, and `active`."""
    import mpmath as mp
    active = [i for i in range(len(rho)) if float(rho[i]) > rho_min]
    with mp.workdps(dps):
        p = _mp_vars(rho, gamma, active)
        m = len(p)
        h = [abs(v) * mp.mpf(rel) for v in p]

        def E(shifts):
            q = list(p)
            for k, s in shifts:
                q[k] += s * h[k]
            return _mp_eval(coords, w, b, C, active, q, len(rho), dps)

        e0 = E(())
        H = mp.zeros(m, m)
        for i in range(m):
            H[i, i] = (E(((i, 1),)) - 2 * e0 + E(((i, -1),))) / (h[i] * h[i])
            for j in range(i):
                v = (E(((i, 1), (j, 1))) - E(((i, 1), (j, -1))) - E(((i, -1), (j, 1))) +
                     E(((i, -1), (j, -1)))) / (4 * h[i] * h[j])
                H[i, j] = H[j, i] = v
        return H, active


# ---------------------------------------------------------------- (b) complex-safe NumPy, AO level
def np_energy_points(coords, w, rho, gamma, b, C, mask):
    idx = np.nonzero(mask)[0]
    r, g, ww, xyz = rho[idx], gamma[idx], w[idx], coords[idx]
    beta = (3.0 / b ** 2) ** 0.75 / 32.0
    om = np.sqrt(C * g ** 2 / r ** 4 + 4.0 * np.pi / 3.0 * r)
    ka = b * 1.5 * np.pi * (9.0 * np.pi) ** (-1.0 / 6.0) * r ** (1.0 / 6.0)
    d = xyz[:, None, :] - xyz[None, :, :]
    R2 = (d * d).sum(-1)
    gij = om[:, None] * R2 + ka[:, None]
    gji = om[None, :] * R2 + ka[None, :]
    phi = -1.5 / (gij * gji * (gij + gji))
    a = ww * r
    return (a * (beta + 0.5 * (phi @ a))).sum()


def np_density(ao, dm):
    rho = np.einsum('gm,mn,gn->g', ao[0], dm, ao[0])
    grad = np.einsum('cgm,mn,gn->cg', ao[1:4], dm, ao[0]) + np.einsum('gm,mn,cgn->cg', ao[0], dm, ao[1:4])
    return rho, grad


def np_energy_ao(ao, coords, w, dm, b, C, mask):
    """E_nlc of a (complex) density matrix; the mask is given (fixed from the real ground state)."""
    rho, grad = np_density(ao, dm)
    return np_energy_points(coords, w, rho, (grad * grad).sum(0), b, C, mask)


# ---------------------------------------------------------------- (c) analytic second derivative
def hess_terms(coords, w, rho, gamma, b, C, rho_min=RHO_MIN):
    """Ground-state data of the second derivative on the active points: per-point parameters and
    their derivatives, the pair matrices and the per-point sums
    (F, U, W, S0, S1, S2) = (sum a phi, -sum a phi_x / 1.5, -sum a phi_x R^2 / 1.5,
                             sum a phi_xx, sum a phi_xx R^2, sum a phi_xx R^4)."""
    mask = rho > rho_min
    idx = np.nonzero(mask)[0]
    r, g, ww, xyz = rho[idx], gamma[idx], w[idx], coords[idx]
    c43 = 4.0 * np.pi / 3.0
    ka = b * 1.5 * np.pi * (9.0 * np.pi) ** (-1.0 / 6.0) * r ** (1.0 / 6.0)
    q = C * g ** 2 / r ** 4 + c43 * r
    om = np.sqrt(q)
    q_r, q_g = -4 * C * g ** 2 / r ** 5 + c43, 2 * C * g / r ** 4
    q_rr, q_rg, q_gg = 20 * C * g ** 2 / r ** 6, -8 * C * g / r ** 5, 2 * C / r ** 4
    t = dict(idx=idx, n=len(rho), w=ww, a=ww * r, ka=ka, om=om)
    t["ka_r"], t["ka_rr"] = ka / (6 * r), -5 * ka / (36 * r * r)
    t["om_r"], t["om_g"] = q_r / (2 * om), q_g / (2 * om)
    t["om_rr"] = q_rr / (2 * om) - q_r * q_r / (4 * om ** 3)
    t["om_rg"] = q_rg / (2 * om) - q_r * q_g / (4 * om ** 3)
    t["om_gg"] = q_gg / (2 * om) - q_g * q_g / (4 * om ** 3)
    d = xyz[:, None, :] - xyz[None, :, :]
    R2 = (d * d).sum(-1)
    x = om[:, None] * R2 + ka[:, None]
    y = x.T
    s = x + y
    phi = -1.5 / (x * y * s)
    ux, uy, us = 1 / x + 1 / s, 1 / y + 1 / s, 1 / s
    t["R2"], t["phi"] = R2, phi
    t["phx"], t["phy"] = -phi * ux, -phi * uy
    t["phxy"] = phi * (ux * uy + us * us)
    phxx = phi * (ux * ux + 1 / (x * x) + us * us)
    a = t["a"]
    t["F"] = phi @ a
    t["P"] = t["phx"] @ a
    t["Q"] = (t["phx"] * R2) @ a
    t["S0"], t["S1"], t["S2"] = phxx @ a, (phxx * R2) @ a, (phxx * R2 * R2) @ a
    return t


def ground_sums(coords, w, rho, gamma, b, C, rho_min=RHO_MIN):
    """(6, G): F, U, W, S0, S1, S2 per point (zero at masked points) -- xt_vv10_ground's output."""
    t = hess_terms(coords, w, rho, gamma, b, C, rho_min)
    out = np.zeros((6, len(rho)))
    out[:, t["idx"]] = [t["F"], t["P"] / 1.5, t["Q"] / 1.5, t["S0"], t["S1"], t["S2"]]
    return out


def first_derivatives(coords, w, rho, gamma, b, C, rho_min=RHO_MIN, t=None):
    t = t or hess_terms(coords, w, rho, gamma, b, C, rho_min)
    beta = (3.0 / b ** 2) ** 0.75 / 32.0
    vr, vg = np.zeros(len(rho)), np.zeros(len(rho))
    vr[t["idx"]] = t["w"] * (beta + t["F"]) + t["a"] * (t["P"] * t["ka_r"] + t["Q"] * t["om_r"])
    vg[t["idx"]] = t["a"] * t["Q"] * t["om_g"]
    return vr, vg


def hess_apply(coords, w, rho, gamma, b, C, rho1, gamma1, rho_min=RHO_MIN, t=None):
    """(vrho1, vgamma1) = d^2 E / d(rho, gamma)^2 applied to (rho1, gamma1), each (nz, G)."""
    t = t or hess_terms(coords, w, rho, gamma, b, C, rho_min)
    idx, a, R2 = t["idx"], t["a"], t["R2"]
    d1, g1 = np.atleast_2d(rho1)[:, idx], np.atleast_2d(gamma1)[:, idx]
    da, dk, dom = t["w"] * d1, t["ka_r"] * d1, t["om_r"] * d1 + t["om_g"] * g1
    s1, s2, s3 = da, a * dk, a * dom
    pa = s1 @ t["phi"].T + s2 @ t["phy"].T + s3 @ (t["phy"] * R2).T
    pk = a * (s1 @ t["phx"].T + s2 @ t["phxy"].T + s3 @ (t["phxy"] * R2).T)
    pw = a * (s1 @ (t["phx"] * R2).T + s2 @ (t["phxy"] * R2).T + s3 @ (t["phxy"] * R2 * R2).T)
    dEa = pa + t["P"] * dk + t["Q"] * dom
    dEk = t["P"] * da + pk + a * (t["S0"] * dk + t["S1"] * dom)
    dEw = t["Q"] * da + pw + a * (t["S1"] * dk + t["S2"] * dom)
    Ek, Ew = a * t["P"], a * t["Q"]
    vr = np.zeros((d1.shape[0], t["n"]))
    vg = np.zeros((d1.shape[0], t["n"]))
    vr[:, idx] = (t["w"] * dEa + t["ka_r"] * dEk + t["om_r"] * dEw + Ek * t["ka_rr"] * d1 +
                  Ew * (t["om_rr"] * d1 + t["om_rg"] * g1))
    vg[:, idx] = t["om_g"] * dEw + Ew * (t["om_rg"] * d1 + t["om_gg"] * g1)
    return vr, vg


def response_ao(ao, coords, w, dm0, dm1, b, C, rho_min=RHO_MIN, t=None):
    """The AO response matrix of the first-order density matrix dm1 (any real matrix) at the
    ground-state total density matrix dm0 (the host statement of get_vnlc_resp's role):
    V1_mn = sum_i [ vrho1 phi_m phi_n + (2 vgamma1 grad rho0 + 2 dE/dgamma grad rho1) . grad(phi_m phi_n) ]."""
    rho0, grad0 = np_density(ao, dm0)
    gamma0 = (grad0 * grad0).sum(0)
    t = t or hess_terms(coords, w, rho0, gamma0, b, C, rho_min)     # t: the terms of dm0, reused over dm1
    rho1, grad1 = np_density(ao, dm1)
    gamma1 = 2.0 * (grad0 * grad1).sum(0)
    vr1, vg1 = hess_apply(coords, w, rho0, gamma0, b, C, rho1, gamma1, rho_min, t)
    _, vg = first_derivatives(coords, w, rho0, gamma0, b, C, rho_min, t)
    wvec = 2.0 * vg1[0] * grad0 + 2.0 * vg * grad1
    aow = 0.5 * vr1[0][:, None] * ao[0] + np.einsum('cg,cgm->gm', wvec, ao[1:4])
    v = ao[0].T @ aow
    return v + v.T
