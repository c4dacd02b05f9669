"""NumPy restatement of the UKS ground-state gradient on a grid held fixed in space (TEST
INFRASTRUCTURE ONLY; not a test file).

Written from the equations, sharing no code with the kernel ``xt_grad_xc``:

* ``ao_deriv2`` -- values, first and second derivatives of the normalised spherical AOs in closed
  form.  A Cartesian Gaussian is a sum over primitives of a product of one-dimensional factors
  u(t) = t^i exp(-a t^2), with

      u'  = (i t^(i-1) - 2a t^(i+1)) exp(-a t^2)
      u'' = (i (i-1) t^(i-2) - 2a (2i+1) t^i + 4a^2 t^(i+2)) exp(-a t^2);

  the spherical transform and the norms are those of ``qc.gto`` (``_sph_transform``, ``_norm``).
* ``xc_bracket`` -- for given h, e, c the sum the kernel forms,

      B[A, x] = sum_s sum_g sum_{mu on A} d_x phi_mu e_s[mu, g] + sum_k h_s[k, g] d_x d_k phi_mu c_s[mu, g],

  by ``einsum``, and S = the sum of the absolute values of every summed term.
* ``uks_grad`` -- dE/dR of a converged UKS (LDA / GGA, pure or global hybrid) with the grid points
  and weights held fixed: the host one-electron terms and the dense derivative ERIs of
  ``tests/grad_ref.py`` plus -2 B with h = w vxc (``xc.eval_xc_eff``, "eff" layout, nothing halved),
  b_s = h_s[0] phi + sum_k h_s[k] d_k phi, e_s = b_s D_s, c_s = phi D_s.
"""
from __future__ import annotations

import numpy as np

import grad_ref as R
from xtddft_amd.qc import xc as _xc
from xtddft_amd.qc.gto import _sph_transform

# order of the second-derivative planes of ao_deriv2: planes 4..9
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
PAIR_INDEX = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def coarse_grids(mol, stride):
    """Every ``stride``-th point of the molecular grid with its weight times ``stride``: a cheap
    grid for the frozen-grid finite differences, where any fixed set of points and weights gives
    a smooth energy whose derivative the ``grid_response = False`` gradient is (only level 3 is
    tabulated in ``qc.grid``)."""
    from xtddft_amd.qc.grid import Grids, gen_grids
    g = gen_grids(mol)
    return Grids(coords=g.coords[::stride].copy(), weights=g.weights[::stride] * float(stride),
                 atom_grid_sizes=g.atom_grid_sizes)


def _u(t, i, a, n):
    """n-th derivative (0, 1, 2) of t^i exp(-a t^2); t (G,), a (P,) -> (P, G)."""
    t = t[None, :]
    a = a[:, None]
    ex = np.exp(-a * t * t)

    def pw(k):
        return t ** k if k >= 0 else np.zeros_like(t)
    if n == 0:
        return pw(i) * ex
    if n == 1:
        return (i * pw(i - 1) - 2 * a * pw(i + 1)) * ex
    return (i * (i - 1) * pw(i - 2) - 2 * a * (2 * i + 1) * pw(i) + 4 * a * a * pw(i + 2)) * ex


def ao_deriv2(mol, coords):
    """(10, G, nao): value, d/dx, d/dy, d/dz, then the second derivatives in the order of ``PAIRS``
    (xx, xy, xz, yy, yz, zz) of the normalised spherical AOs of ``mol`` (a ``Mole`` or a
    ``grad_ref.ShellMol``) at ``coords`` (G, 3)."""
    coords = np.asarray(coords, dtype=np.float64)
    G = coords.shape[0]
    out = np.zeros((10, G, mol.nao))
    orders = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)] + \
        [tuple(int(d == i) + int(d == j) for d in range(3)) for i, j in PAIRS]
    for s, p0 in zip(mol.shells, mol.ao_loc[:-1]):
        l = s.l
        r = coords - np.asarray(s.center)[None, :]
        a = np.asarray(s.exps, dtype=np.float64)
        cf = np.asarray(s.coefs, dtype=np.float64)
        comps = [(ix, iy, l - ix - iy) for ix in range(l, -1, -1) for iy in range(l - ix, -1, -1)]
        cart = np.zeros((10, G, len(comps)))
        for k, pw in enumerate(comps):
            # per direction and derivative order: (P, G)
            u = [[_u(r[:, d], pw[d], a, n) for n in range(3)] for d in range(3)]
            for q, od in enumerate(orders):
                cart[q, :, k] = np.einsum('p,pg->g', cf, u[0][od[0]] * u[1][od[1]] * u[2][od[2]])
        T = _sph_transform(l) * mol._norm[p0:p0 + 2 * l + 1, None]
        out[:, :, p0:p0 + 2 * l + 1] = np.einsum('qgk,mk->qgm', cart, T)
    return out


def xc_bracket(ao10, ao_atom, natm, h, e, c, gga):
    """(B (natm, 3), S): the kernel's sum and the sum of |terms|.  ao10 (10, G, nao) from
    ``ao_deriv2``; h (nspin, 4, G); e, c (nspin, nao, G) (c and h[:, 1:] unused when not gga)."""
    d1 = ao10[1:4]                                                  # (x, G, mu)
    t = np.einsum('xgm,smg->xm', d1, e)
    S = float(np.einsum('xgm,smg->', np.abs(d1), np.abs(e)))
    if gga:
        d2 = ao10[4:][PAIR_INDEX]                                   # (x, k, G, mu)
        t = t + np.einsum('xkgm,skg,smg->xm', d2, h[:, 1:4], c, optimize=True)
        S += float(np.einsum('xkgm,skg,smg->', np.abs(d2), np.abs(h[:, 1:4]), np.abs(c), optimize=True))
    B = np.stack([t[:, np.asarray(ao_atom) == A].sum(axis=1) for A in range(natm)])
    return B, S


def xc_operands(mol, coords, weights, xc, dms, ao10=None):
    """(ao10, h (2, 4, G), e (2, nao, G), c (2, nao, G), gga) at the spin densities dms on the host."""
    ao10 = ao_deriv2(mol, coords) if ao10 is None else ao10
    gga = _xc.xc_type(xc) == "GGA"
    G = ao10.shape[1]
    c = np.einsum('gn,snm->smg', ao10[0], dms)                      # c_s = phi D_s
    rho = np.zeros((2, 4 if gga else 1, G))
    rho[:, 0] = np.einsum('gm,smg->sg', ao10[0], c)
    if gga:
        rho[:, 1:] = 2.0 * np.einsum('kgm,smg->skg', ao10[1:4], c)
    vxc = _xc.eval_xc_eff(xc, rho, deriv=1)[1]
    h = np.zeros((2, 4, G))
    h[:, :vxc.shape[1]] = vxc * np.asarray(weights)[None, None, :]
    b = np.einsum('sg,gn->sgn', h[:, 0], ao10[0])
    if gga:
        b = b + np.einsum('skg,kgn->sgn', h[:, 1:], ao10[1:4])
    e = np.einsum('sgn,snm->smg', b, dms)
    return ao10, h, e, c, gga


def uks_grad(mf, ip=None):
    """(dE/dR (natm, 3), S, parts) of a converged UKS with the grid held fixed; ``ip``: the dense
    derivative ERIs (``grad_ref.deriv_eri``).  S is the sum of the absolute values of the summed
    terms (one-electron, two-electron and nuclear parts by component, the XC part by grid term);
    parts: the XC gradient and the sum over atoms of the whole gradient (zero only to the extent
    the grid is converged: the weight derivatives are absent)."""
    mol = mf.mol
    ip = R.deriv_eri(mol) if ip is None else ip
    f = mf.get_hcore()[None] + np.asarray(mf._veff)
    d, w = [], 0.0
    for s in range(2):
        co = mf.mo_coeff[s][:, mf.mo_occ[s] > 0]
        d.append(co @ co.T)
        w = w + co @ (co.T @ f[s] @ co) @ co.T
    hyb = float(mf.hyb)
    pairs = [(1, 0, d[0] + d[1], d[0] + d[1])]
    if hyb != 0:
        pairs += [(0, -hyb, d[0], d[0]), (0, -hyb, d[1], d[1])]
    g1, g2, gn = R._de_1e(mol, d[0] + d[1], w), R._de_2e(mol, ip, pairs), R._nuc(mol)
    ao10, h, e, c, gga = xc_operands(mol, mf.grids.coords, mf.grids.weights, mf.xc, np.asarray(d))
    B, Sx = xc_bracket(ao10, mol.ao_atom(), mol.natm, h, e, c, gga)
    gx = -2.0 * B
    g = g1 + g2 + gn + gx
    S = float(np.abs(g1).sum() + np.abs(g2).sum() + np.abs(gn).sum() + 2.0 * Sx)
    return g, S, dict(xc=gx, sum_atoms=g.sum(axis=0))
