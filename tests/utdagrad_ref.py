"""NumPy restatement of the U-TDA (spin-conserving TDA) gradient on a UHF or UKS reference, on a grid
held fixed in space (TEST INFRASTRUCTURE ONLY; not a test file).

Written from the equations in a formulation the device code does not share: the dense derivative
ERIs of ``tests/grad_ref.py``, the closed-form AO derivatives of ``tests/ksgrad_ref.py``, the
pointwise response and the XC bracket of ``tests/sfksgrad_ref.py``, the U-TDA A matrix from MO
integrals and MO values on the grid, a dense ``solve`` of the Z-vector equations, the two-electron
density pairs un-merged (X_S and X_A apart, ground state and T + Z^S as cross terms), and the third
functional derivative as an explicit tensor (three nested autograd passes over every component), where
the package takes two directional derivatives and one backward pass.

The functional that is differentiated, with X_s (nvir_s, nocc_s), |X_a|^2 + |X_b|^2 = 1,
Xt_s = C_v X_s C_o^T, X_S = (Xt + Xt^T) / 2, X_A = (Xt - Xt^T) / 2:

    omega = sum_s tr(X_s^T F_vv X_s) - tr(X_s F_oo X_s^T) + X_S,tot : J[X_S,tot]
            - hyb sum_s (X_S,s : K[X_S,s] + X_A,s : K[X_A,s]) + sum_g w rho1^T fxc rho1,   rho1 = rho[X_S]

Everything stays in the order alpha, beta.  Next to the gradient comes S, the same sum with every
part replaced by its absolute value.
"""
from __future__ import annotations

import numpy as np

import grad_ref as R
import sfksgrad_ref as SK
from xtddft_amd.qc import xc as _xc


def xc_third(xc, rho):
    """kxc (2, nc, 2, nc, 2, nc, G): the third derivative of the energy density with respect to the
    "eff" variables at the spin densities rho (2, nc, G), zero where ``eval_xc_eff`` screens the point."""
    import torch
    rho = np.asarray(rho, dtype=np.float64)
    nc, G = rho.shape[1], rho.shape[2]
    out = np.zeros((2 * nc, 2 * nc, 2 * nc, G))
    mask = (rho[0, 0] + rho[1, 0]) > _xc.DENS_THRESHOLD
    if not mask.any():
        return out.reshape(2, nc, 2, nc, 2, nc, G)
    x = torch.tensor(rho[:, :, mask].reshape(2 * nc, -1), dtype=torch.float64, requires_grad=True)
    eps = _xc.energy_density_torch(xc, x.reshape(2, nc, -1))
    g = torch.autograd.grad(eps.sum(), x, create_graph=True)[0]
    n = 2 * nc
    sub = np.zeros((n, n, n, int(mask.sum())))
    for k in range(n):
        hk = torch.autograd.grad(g[k].sum(), x, create_graph=True)[0]
        for l in range(n):
            if not hk[l].requires_grad:
                continue
            t = torch.autograd.grad(hk[l].sum(), x, retain_graph=True, allow_unused=True)[0]
            if t is not None:
                sub[k, l] = t.detach().numpy()
    # exact symmetry in the three indices (autograd round-off)
    sub = (sub + sub.transpose(0, 2, 1, 3) + sub.transpose(1, 0, 2, 3) + sub.transpose(1, 2, 0, 3)
           + sub.transpose(2, 0, 1, 3) + sub.transpose(2, 1, 0, 3)) / 6.0
    out[..., mask] = sub
    return out.reshape(2, nc, 2, nc, 2, nc, G)


def rho0_of(mf, xa):
    """The SCF spin densities (2, nc, G) on the grid of the XC arrays."""
    d0 = SK._d0(mf)
    nc = 4 if xa.gga else 1
    c = np.einsum('gn,snm->sgm', xa.ao10[0], d0)
    rho = np.zeros((2, nc, xa.w.size))
    rho[:, 0] = np.einsum('gm,sgm->sg', xa.ao10[0], c)
    if xa.gga:
        rho[:, 1:] = 2.0 * np.einsum('kgm,sgm->skg', xa.ao10[1:4], c)
    return rho


def kxc_arrays(mf, xa):
    return xc_third(mf.xc, rho0_of(mf, xa))


def zero_kxc():
    return np.zeros((2, 4, 2, 4, 2, 4, 1))


def potential(xa, wv):
    """(2, nao, nao): the potentials of the weights wv (2, 4, G), unhalved, one per channel."""
    ao = xa.ao10
    if xa.gga:
        b = 0.5 * wv[:, 0][:, :, None] * ao[0][None] + np.einsum('skg,kgm->sgm', wv[:, 1:], ao[1:4])
        v = np.einsum('gm,sgn->smn', ao[0], b)
        return v + v.transpose(0, 2, 1)
    return np.einsum('gm,sg,gn->smn', ao[0], wv[:, 0], ao[0])


def _orbitals(mf):
    o = [mf.mo_coeff[s][:, mf.mo_occ[s] > 0] for s in range(2)]
    v = [mf.mo_coeff[s][:, mf.mo_occ[s] == 0] for s in range(2)]
    return o, v


# ------------------------------------------------------------------ states
def utda_states(mf, xa=None, hyb=None):
    """(omega ascending, [(X_a (nvir_a, nocc_a), X_b (nvir_b, nocc_b))] per root) of the U-TDA A matrix
    A[(s a i), (t b j)] = delta (eps_a - eps_i) + (a i|b j) - hyb delta_st (a b|i j) + <a i|w fxc|b j>
    from MO integrals and MO values on the grid; ``xa`` None: no XC part (Hartree-Fock)."""
    hyb = float(getattr(mf, "hyb", 1.0)) if hyb is None else float(hyb)
    eri = SK._eri(mf)
    o, v = _orbitals(mf)
    dims = [v[s].shape[1] * o[s].shape[1] for s in range(2)]
    blocks = [[None, None], [None, None]]
    for s in range(2):
        for t in range(2):
            a = np.einsum('pqrs,pa,qi,rb,sj->aibj', eri, v[s], o[s], v[t], o[t], optimize=True)
            if s == t:
                a = a - hyb * np.einsum('pqrs,pa,qb,ri,sj->aibj', eri, v[s], v[s], o[s], o[s], optimize=True)
            blocks[s][t] = a.reshape(dims[s], dims[t])
    A = np.block(blocks)
    if xa is not None:
        A = A + SK._kxc_matrix(xa, (0, 1), o, v)
    gaps = [(mf.mo_energy[s][mf.mo_occ[s] == 0][:, None] - mf.mo_energy[s][mf.mo_occ[s] > 0][None, :]).ravel()
            for s in range(2)]
    A[np.diag_indices(sum(dims))] += np.hstack(gaps)
    e, vec = np.linalg.eigh(0.5 * (A + A.T))
    xs = [(vec[:dims[0], r].reshape(v[0].shape[1], o[0].shape[1]), vec[dims[0]:, r].reshape(v[1].shape[1], o[1].shape[1]))
          for r in range(vec.shape[1])]
    return e, xs


def xao(mf, x):
    """(2, nao, nao): the AO transition densities C_v X_s C_o^T of one root."""
    o, v = _orbitals(mf)
    return np.asarray([v[s] @ x[s] @ o[s].T for s in range(2)])


def follow(s1e, x0, xs):
    """(root among ``xs`` that is the state ``x0``, its overlap): |sum_s tr(X0_s^T S X_s S)| over the AO
    transition densities of both spins, which does not depend on the phases of the orbitals."""
    ov = np.abs([np.einsum('spq,pr,srt,qt->', x0, s1e, x, s1e, optimize=True) for x in xs])
    k = int(ov.argmax())
    return k, float(ov[k])


def omega_of(mf, x, xa=None, hyb=None):
    """The functional of the module docstring at the amplitudes x (not re-normalised)."""
    hyb = float(getattr(mf, "hyb", 1.0)) if hyb is None else float(hyb)
    eri = SK._eri(mf)
    o, v = _orbitals(mf)
    f_ao = mf.get_hcore()[None] + np.asarray(mf._veff)
    om = 0.0
    for s in range(2):
        om += np.trace(x[s].T @ (v[s].T @ f_ao[s] @ v[s]) @ x[s]) - np.trace(x[s] @ (o[s].T @ f_ao[s] @ o[s]) @ x[s].T)
    dx = xao(mf, x)
    xs, xn = (dx + dx.transpose(0, 2, 1)) / 2, (dx - dx.transpose(0, 2, 1)) / 2
    vj, vk = R._jk(eri, [xs[0] + xs[1], xs[0], xs[1], xn[0], xn[1]])
    om += np.sum((xs[0] + xs[1]) * vj[0])
    om -= hyb * (np.sum(xs[0] * vk[1]) + np.sum(xs[1] * vk[2]) + np.sum(xn[0] * vk[3]) + np.sum(xn[1] * vk[4]))
    if xa is not None:
        c = np.einsum('gn,snm->sgm', xa.ao10[0], xs)
        (rho1, wv, _), _ = SK.resp_arrays(xa.ao10, c, xa.fxc, xa.w, xa.gga)
        om += np.sum(rho1 * wv)
    return float(om)


# ------------------------------------------------------------------ the gradient
def utda_grad(mf, x, ip=None, xa=None, kxc=None, hyb=None, mcache=None):
    """(d(E_SCF + omega)/dR (natm, 3), S, parts) of the U-TDA state with amplitudes x = (X_a, X_b).
    ``xa``: the XC arrays (``sfksgrad_ref.xc_arrays``; ``zero_xc_arrays`` for Hartree-Fock), ``kxc``: the
    third derivative (``kxc_arrays`` / ``zero_kxc``), ``hyb``: the exchange fraction.  ``mcache``: a dict
    that keeps the Z-vector matrix between states.  parts: xc (the XC nuclear-derivative part), xc_kxc
    (what the third derivative adds to it), omega (the functional), sum_atoms, zvector_rhs."""
    mol = mf.mol
    ip = R.deriv_eri(mol) if ip is None else ip
    hyb = float(getattr(mf, "hyb", 1.0)) if hyb is None else float(hyb)
    eri = SK._eri(mf)
    nc = 4 if xa.gga else 1
    C = [mf.mo_coeff[s] for s in range(2)]
    o, v = _orbitals(mf)
    no = [o[s].shape[1] for s in range(2)]
    nv = [v[s].shape[1] for s in range(2)]
    f_ao = mf.get_hcore()[None] + np.asarray(mf._veff)
    F = [C[s].T @ f_ao[s] @ C[s] for s in range(2)]
    nrm = np.sqrt(sum(np.sum(xi * xi) for xi in x))
    x = [np.asarray(xi) / nrm for xi in x]
    too = [-x[s].T @ x[s] for s in range(2)]
    tvv = [x[s] @ x[s].T for s in range(2)]
    dt = np.asarray([v[s] @ tvv[s] @ v[s].T + o[s] @ too[s] @ o[s].T for s in range(2)])
    dt = (dt + dt.transpose(0, 2, 1)) / 2
    dx = xao(mf, x)
    xs, xn = (dx + dx.transpose(0, 2, 1)) / 2, (dx - dx.transpose(0, 2, 1)) / 2
    xst = xs[0] + xs[1]
    vj, vk = R._jk(eri, [dt[0], dt[1], xst, dx[0], dx[1]])
    # the coupling applied to X: J[X_S,tot] - hyb K[Xt_s] + V^resp_s[X_S]
    c = np.einsum('gn,snm->sgm', xa.ao10[0], xs)
    (rho1, wvx, bx), _ = SK.resp_arrays(xa.ao10, c, xa.fxc, xa.w, xa.gga)
    vx = np.einsum('gm,sgn->smn', xa.ao10[0], bx)
    if xa.gga:
        vx = vx + vx.transpose(0, 2, 1)
    G = [vj[2] - hyb * vk[3 + s] + vx[s] for s in range(2)]
    gmo = [C[s].T @ G[s] @ C[s] for s in range(2)]
    # the third derivative: wv2 = w d(rho1^T fxc rho1) / d rho0
    wv2 = np.zeros((2, 4, xa.w.size))
    wv2[:, :nc] = xa.w * np.einsum('skg,sktlumg,tlg->umg', rho1[:, :nc], kxc, rho1[:, :nc], optimize=True)
    ft = SK.vresp_xc(xa, dt)[0]
    vk2 = potential(xa, wv2)
    g0 = [vj[0] + vj[1] - hyb * vk[s] + ft[s] + vk2[s] for s in range(2)]
    rhs = [2 * (v[s].T @ g0[s] @ o[s] + gmo[s][no[s]:, no[s]:].T @ x[s] - x[s] @ gmo[s][:no[s], :no[s]].T)
           for s in range(2)]
    na = nv[0] * no[0]
    dim = na + nv[1] * no[1]

    def split(z):
        return [z[:na].reshape(nv[0], no[0]), z[na:].reshape(nv[1], no[1])]

    def apply(z):                # the J / K and orbital-energy part of the Z-vector operator
        zz = split(z)
        d = [v[s] @ zz[s] @ o[s].T for s in range(2)]
        j, k = R._jk(eri, [(m + m.T) / 2 for m in d])
        w2 = 2 * ((j[0] + j[1])[None] - hyb * k)
        r = [v[s].T @ w2[s] @ o[s] + F[s][no[s]:, no[s]:].T @ zz[s] - zz[s] @ F[s][:no[s], :no[s]].T for s in range(2)]
        return np.hstack((r[0].ravel(), r[1].ravel()))
    if mcache is not None and "M" in mcache:
        M = mcache["M"]
    else:
        M = np.stack([apply(e) for e in np.eye(dim)], axis=1) + 2.0 * SK._kxc_matrix(xa, (0, 1), o, v)
        if mcache is not None:
            mcache["M"] = M
    z = split(np.linalg.solve(M, -np.hstack((rhs[0].ravel(), rhs[1].ravel()))))
    zs = np.asarray([v[s] @ z[s] @ o[s].T for s in range(2)])
    zs = (zs + zs.transpose(0, 2, 1)) / 2
    j, k = R._jk(eri, zs)
    gz = (j[0] + j[1])[None] - hyb * k + SK.vresp_xc(xa, zs)[0]
    W = 0.0
    for s in range(2):
        n = no[s]
        w = np.zeros_like(F[s])
        w[:n, :n] = F[s][:n, :n] + o[s].T @ (g0[s] + gz[s]) @ o[s] + too[s] @ F[s][:n, :n] + x[s].T @ gmo[s][n:, :n]
        w[n:, n:] = tvv[s] @ F[s][n:, n:].T + x[s] @ gmo[s][n:, :n].T
        w[n:, :n] = z[s] @ F[s][:n, :n].T + 2 * x[s] @ gmo[s][:n, :n].T
        W = W + C[s] @ w @ C[s].T
    d0 = np.asarray([o[s] @ o[s].T for s in range(2)])
    p = zs + dt
    d0t, pt, h = d0[0] + d0[1], p[0] + p[1], hyb
    pairs = [(1, 0, d0t, d0t), (0, -h, d0[0], d0[0]), (0, -h, d0[1], d0[1]),
             (1, 0, d0t, pt), (0, -h, d0[0], p[0]), (0, -h, d0[1], p[1]),
             (1, 0, pt, d0t), (0, -h, p[0], d0[0]), (0, -h, p[1], d0[1]),
             (2, 0, xst, xst), (0, -2 * h, xs[0], xs[0]), (0, -2 * h, xs[1], xs[1])]
    g1, g2, gn = R._de_1e(mol, d0t + pt, W), R._de_2e(mol, ip, pairs), R._nuc(mol)
    on = mol.ao_atom()
    for s in range(2):           # -2 hyb vk[X_A][x,p,q] (X_A[p,q] - X_A[q,p])
        vka = -np.einsum('xijkl,jk->xil', ip, xn[s], optimize=True)
        per_ao = -2 * h * np.einsum('xpq,pq->xp', vka, xn[s] - xn[s].T)
        g2 = g2 + np.stack([per_ao[:, on == A].sum(axis=1) for A in range(mol.natm)])
    gx1, s1 = SK.gxc(mol, xa, xa.h0, d0 + p)
    gx2, s2 = SK.gxc(mol, xa, SK.vresp_xc(xa, p)[1], d0)
    gx3, s3 = SK.gxc(mol, xa, 2.0 * wvx, xs)
    gx4, s4 = SK.gxc(mol, xa, wv2, d0)
    g = g1 + g2 + gn + gx1 + gx2 + gx3 + gx4
    S = float(np.abs(g1).sum() + np.abs(g2).sum() + np.abs(gn).sum() + s1 + s2 + s3 + s4)
    return g, S, dict(xc=gx1 + gx2 + gx3 + gx4, xc_kxc=gx4, omega=omega_of(mf, x, xa, hyb), sum_atoms=g.sum(axis=0),
                      zvector_rhs=rhs, wv2=wv2)
