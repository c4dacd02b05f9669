"""VV10 non-local correlation on a quadrature grid (host, NumPy).

The energy, with a_i = w_i rho_i and only points with rho_i > rho_min taking part (the mask
is fixed from the real part of the ground-state density):

    E_nlc = sum_i a_i [ beta + 1/2 sum_j a_j Phi_ij ]            (j = i included)
    Phi_ij = -3/2 / (g_ij g_ji (g_ij + g_ji)),  g_ij = omega0_i R_ij^2 + kappa_i
    omega0 = sqrt(C gamma^2 / rho^4 + (4 pi / 3) rho),  gamma = |grad rho|^2
    kappa  = b (3/2) pi (9 pi)^(-1/6) rho^(1/6),  beta = (3 / b^2)^(3/4) / 32

rho is the total (alpha + beta) density, so the potential is the same for both spins.  The
parameters (b, C) are the caller's; no named sets are kept here.  ``rho_min`` (default 1e-8)
is a choice of this code and is not pinned to PySCF; nor is the grid the term is summed on.

Everything differentiated here is analytic in the density (no ``abs``, no ``where`` on rho or
gamma), so a complex density matrix D0 + i h X differentiates it to rounding (complex step).
The response (second derivative) exists only on the device (csrc/xt_vv10.hip).
"""
from __future__ import annotations

import numpy as np

KAPPA_PREF = 1.5 * np.pi * (9.0 * np.pi) ** (-1.0 / 6.0)
FOUR_PI_3 = 4.0 * np.pi / 3.0
RHO_MIN = 1e-8
_ROWS = 512   # target rows per block of the pair sum


def beta_of(b):
    return (3.0 / (b * b)) ** 0.75 / 32.0


def point_params(rho, gamma, b, C):
    """kappa, omega0 and their first derivatives (kappa_rho, omega_rho, omega_gamma)."""
    kappa = b * KAPPA_PREF * rho ** (1.0 / 6.0)
    omega = np.sqrt(C * gamma * gamma / rho ** 4 + FOUR_PI_3 * rho)
    kappa_r = kappa / (6.0 * rho)
    omega_r = (-4.0 * C * gamma * gamma / rho ** 5 + FOUR_PI_3) / (2.0 * omega)
    omega_g = (2.0 * C * gamma / rho ** 4) / (2.0 * omega)
    return kappa, omega, kappa_r, omega_r, omega_g


def gen_nlc_grids(mol, n_rad, n_ang, prune=True):
    """The VV10 grid: per atom ``atomic_grid(z, n_rad, n_ang)``, Becke-partitioned (``qc.grid``).
    The counts are the caller's; this is not PySCF's ``nlcgrids`` level."""
    from .grid import Grids, atomic_grid, becke_partition
    xyz, charges = mol.atom_coords(), mol.atom_charges()
    coords, weights, owner, sizes = [], [], [], []
    for ia, z in enumerate(charges):
        c, w, angs = atomic_grid(int(z), n_rad, n_ang, prune=prune)
        coords.append(c + xyz[ia])
        weights.append(w)
        owner.append(np.full(w.size, ia))
        sizes.append((int(angs.size), angs))
    coords = np.concatenate(coords)
    weights = np.concatenate(weights) * becke_partition(xyz, charges, coords, np.concatenate(owner))
    return Grids(coords=coords, weights=weights, atom_grid_sizes=sizes)


def _device_sums(xyz, w, r, gm, b, C, device):
    """F, U, W of the (already unmasked, real) points from the library's xt_vv10_ground."""
    import torch
    from .. import _capi
    L = _capi.lib()
    dv = torch.device(f"cuda:{device}")
    n = len(r)
    with torch.cuda.device(dv):
        t = [torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device=dv) for x in (xyz, w, r, gm)]
        sums = torch.zeros((6, n), dtype=torch.float64, device=dv)
        _capi.check(L.xt_vv10_ground(n, *[x.data_ptr() for x in t], float(b), float(C), 0.0, 0, n,
                                     sums.data_ptr(), torch.cuda.current_stream(dv).cuda_stream), "xt_vv10_ground")
        s = sums.cpu().numpy()
    return s[0], s[1], s[2]


def ground(coords, weights, rho, gamma, b, C, rho_min=RHO_MIN, mask=None, device=None):
    """E_nlc, dE/drho_i, dE/dgamma_i and the per-point pair sums
        F_i = -3/2 sum_j T_ij,  U_i = sum_j T_ij (1/g_ij + 1/(g_ij + g_ji)),
        W_i = sum_j R_ij^2 T_ij (1/g_ij + 1/(g_ij + g_ji)),  T_ij = a_j / (g_ij g_ji (g_ij + g_ji)),
    as a dict of arrays over all points (zero at masked points).  ``device``: take the pair
    sums from the library on that GPU (real densities only); None: NumPy."""
    rho = np.asarray(rho)
    gamma = np.asarray(gamma)
    if mask is None:
        mask = rho.real > rho_min
    idx = np.nonzero(mask)[0]
    r, gm, w = rho[idx], gamma[idx], np.asarray(weights)[idx]
    xyz = np.asarray(coords, dtype=float)[idx]
    kappa, omega, kappa_r, omega_r, omega_g = point_params(r, gm, b, C)
    a = w * r
    n = len(idx)
    dt = np.result_type(rho.dtype, gamma.dtype, float)
    F = np.zeros(n, dt)
    U = np.zeros(n, dt)
    W = np.zeros(n, dt)
    if device is not None and n > 0:
        F, U, W = _device_sums(xyz, w, r, gm, b, C, device)
    else:
        for i0 in range(0, n, _ROWS):
            s = slice(i0, min(n, i0 + _ROWS))
            d = xyz[s, None, :] - xyz[None, :, :]
            R2 = np.einsum('ijx,ijx->ij', d, d)
            x = omega[s, None] * R2 + kappa[s, None]
            y = omega[None, :] * R2 + kappa[None, :]
            xy = x + y
            T = a[None, :] / (x * y * xy)
            Tu = T * (1.0 / x + 1.0 / xy)
            F[s] = -1.5 * T.sum(1)
            U[s] = Tu.sum(1)
            W[s] = (R2 * Tu).sum(1)
    beta = beta_of(b)
    out = {"mask": mask, "E": (a * (beta + 0.5 * F)).sum()}
    vrho = w * (beta + F + 1.5 * r * (U * kappa_r + W * omega_r))
    vgamma = w * 1.5 * r * W * omega_g
    for k, v in (("vrho", vrho), ("vgamma", vgamma), ("F", F), ("U", U), ("W", W)):
        full = np.zeros(len(rho), dt)
        full[idx] = v
        out[k] = full
    return out


def density(ao, dm):
    """rho and grad rho (3, G) of a density matrix on AO values ao (4, G, nao); dm may be
    non-symmetric and complex (its symmetric part is what the density sees)."""
    ds = 0.5 * (dm + dm.T)
    c0 = ao[0] @ ds
    rho = np.einsum('gm,gm->g', c0, ao[0])
    grad = 2.0 * np.einsum('gm,cgm->cg', c0, ao[1:4])
    return rho, grad


def nlc_vmat(ao, coords, weights, dm, b, C, rho_min=RHO_MIN, mask=None, device=None):
    """E_nlc and the AO matrix V_nlc = dE_nlc / dD of the total density matrix dm:
    V_mn = sum_i [ vrho_i phi_m phi_n + 2 vgamma_i grad rho . grad(phi_m phi_n) ]."""
    rho, grad = density(ao, dm)
    gamma = (grad * grad).sum(0)
    g = ground(coords, weights, rho, gamma, b, C, rho_min, mask, device)
    aow = 0.5 * g["vrho"][:, None] * ao[0] + np.einsum('cg,cgm->gm', 2.0 * g["vgamma"] * grad, ao[1:4])
    v = ao[0].T @ aow
    return g["E"], v + v.T
