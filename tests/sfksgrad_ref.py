"""NumPy restatement of the collinear spin-flip TDA gradient on a UKS reference, on a grid held
fixed in space (TEST INFRASTRUCTURE ONLY; not a test file).

Written from the equations in a formulation the device code does not share: the dense derivative
ERIs of ``tests/grad_ref.py``, the closed-form AO first and second derivatives of
``tests/ksgrad_ref.py``, the host ``xc.eval_xc_eff(..., deriv=2)``, plain ``einsum`` for rho1, wv and
V^resp, the collinear spin-flip A matrix from MO integrals, and a dense ``solve`` of the Z-vector
equations (no iteration).  What it shares with the package: the one-electron derivatives
(``grad_ref._de_1e``) and, as the same equations, the block structure of W.

Labels as in ``xtddft_amd/grad.py``: "a" is the flipped-from spin, "b" the flipped-to spin; the XC
arrays stay in the order alpha, beta and every density pair is put into that order before it meets
them.  Next to every summed quantity comes S, the same expression with every term replaced by its
absolute value.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import grad_ref as R
import ksgrad_ref as K
from xtddft_amd.qc import xc as _xc

# ao10 (10, G, nao) of ksgrad_ref.ao_deriv2; w (G,); h0 = w vxc[rho0] (2, 4, G) unhalved; fxc
# (2, nc, 2, nc, G) with nc = 4 (gga) or 1; all in the order alpha, beta
XCArrays = namedtuple("XCArrays", "ao10 w h0 fxc gga")


def xc_arrays(mf, ao10=None):
    """The XC arrays at the SCF density of a converged UKS (LDA / GGA) on its own grid."""
    ao10 = K.ao_deriv2(mf.mol, mf.grids.coords) if ao10 is None else ao10
    gga = _xc.xc_type(mf.xc) == "GGA"
    d0 = _d0(mf)
    w = np.asarray(mf.grids.weights, dtype=np.float64)
    c = np.einsum('gn,snm->sgm', ao10[0], d0)
    rho = np.zeros((2, 4 if gga else 1, w.size))
    rho[:, 0] = np.einsum('gm,sgm->sg', ao10[0], c)
    if gga:
        rho[:, 1:] = 2.0 * np.einsum('kgm,sgm->skg', ao10[1:4], c)
    _, vxc, fxc = _xc.eval_xc_eff(mf.xc, rho, deriv=2)
    h0 = np.zeros((2, 4, w.size))
    h0[:, :vxc.shape[1]] = vxc * w
    return XCArrays(ao10, w, h0, fxc, gga)


def zero_xc_arrays(nao):
    """No functional at all: one grid point of weight zero (the Hartree-Fock limit)."""
    return XCArrays(np.zeros((10, 1, nao)), np.zeros(1), np.zeros((2, 4, 1)), np.zeros((2, 4, 2, 4, 1)), True)


def _eri(mf):
    """The stored four-index integrals as a host array."""
    e = mf.eri
    return e.cpu().numpy() if hasattr(e, "cpu") else np.asarray(e)


def _d0(mf):
    return np.asarray([mf.mo_coeff[s][:, mf.mo_occ[s] > 0] @ mf.mo_coeff[s][:, mf.mo_occ[s] > 0].T for s in range(2)])


# ------------------------------------------------------------------ the pointwise response
def resp_arrays(ao, c, fxc, w, gga):
    """What ``xt_xc_resp`` forms from c_s = phi dm_s: ((rho1, wv, b), (S_rho1, S_wv, S_b)).  ao
    (>= nc, G, nao), c (2, G, nao), fxc (2, nc, 2, nc, G), w (G,); rho1, wv (2, 4, G) (planes 1..3
    zero for LDA), b (2, G, nao) with the half on component 0 for GGA."""
    nc = 4 if gga else 1
    G = c.shape[1]
    aa, ca = np.abs(ao), np.abs(c)
    rho1, s_rho = np.zeros((2, 4, G)), np.zeros((2, 4, G))
    rho1[:, 0] = np.einsum('gm,sgm->sg', ao[0], c)
    s_rho[:, 0] = np.einsum('gm,sgm->sg', aa[0], ca)
    if gga:
        rho1[:, 1:] = 2.0 * np.einsum('kgm,sgm->skg', ao[1:4], c)
        s_rho[:, 1:] = 2.0 * np.einsum('kgm,sgm->skg', aa[1:4], ca)
    wv, s_wv = np.zeros((2, 4, G)), np.zeros((2, 4, G))
    wv[:, :nc] = w * np.einsum('skrlg,rlg->skg', fxc, rho1[:, :nc])
    s_wv[:, :nc] = np.abs(w) * np.einsum('skrlg,rlg->skg', np.abs(fxc), s_rho[:, :nc])
    if gga:
        b = 0.5 * wv[:, 0][:, :, None] * ao[0][None] + np.einsum('skg,kgm->sgm', wv[:, 1:], ao[1:4])
        s_b = 0.5 * s_wv[:, 0][:, :, None] * aa[0][None] + np.einsum('skg,kgm->sgm', s_wv[:, 1:], aa[1:4])
    else:
        b = wv[:, 0][:, :, None] * ao[0][None]
        s_b = s_wv[:, 0][:, :, None] * aa[0][None]
    return (rho1, wv, b), (s_rho, s_wv, s_b)


def vresp_xc(xa, dm):
    """(V^resp (2, nao, nao), wv (2, 4, G), S_V, S_wv) of a symmetric density pair (alpha, beta)."""
    ao = xa.ao10
    dm = np.asarray(dm)
    c = np.einsum('gn,snm->sgm', ao[0], dm)
    sc = np.einsum('gn,snm->sgm', np.abs(ao[0]), np.abs(dm))
    (_, wv, b), (_, s_wv, s_b) = resp_arrays(ao, c, xa.fxc, xa.w, xa.gga)
    # S with the rounding of c itself counted: |ao| |dm| in place of |c|
    (_, _, _), (_, s_wv, s_b) = resp_arrays(np.abs(ao), sc, np.abs(xa.fxc), np.abs(xa.w), xa.gga)
    v = np.einsum('gm,sgn->smn', ao[0], b)
    s_v = np.einsum('gm,sgn->smn', np.abs(ao[0]), s_b)
    if xa.gga:
        v, s_v = v + v.transpose(0, 2, 1), s_v + s_v.transpose(0, 2, 1)
    return v, wv, s_v, s_wv


def gxc(mol, xa, h, dm):
    """(G_xc[h; D] (natm, 3), S): -2 x the bracket of ``ksgrad_ref.xc_bracket`` with the weights h
    (2, 4, G) unhalved and the symmetric densities dm (alpha, beta)."""
    ao = xa.ao10
    dm = np.asarray(dm)
    c = np.einsum('gn,snm->smg', ao[0], dm)
    b = np.einsum('sg,gn->sgn', h[:, 0], ao[0])
    if xa.gga:
        b = b + np.einsum('skg,kgn->sgn', h[:, 1:], ao[1:4])
    e = np.einsum('sgn,snm->smg', b, dm)
    B, S = K.xc_bracket(ao, mol.ao_atom(), mol.natm, h, e, c, xa.gga)
    return -2.0 * B, 2.0 * S


# ------------------------------------------------------------------ states
def sf_states(mf, isf, hyb=None):
    """(omega ascending, x (root, nvir_f, nocc_i)) of the collinear spin-flip A matrix from MO
    integrals: A[ia, jb] = delta_ij delta_ab (eps^f_a - eps^i_i) - hyb (ij|ab), i, j occupied
    orbitals of the flipped-from spin, a, b virtuals of the flipped-to spin."""
    hyb = float(mf.hyb) if hyb is None else hyb
    s = (0, 1) if isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    eo = mf.mo_energy[s[0]][mf.mo_occ[s[0]] > 0]
    ev = mf.mo_energy[s[1]][mf.mo_occ[s[1]] == 0]
    no, nv = co.shape[1], cv.shape[1]
    ijab = np.einsum('pqrs,pi,qj,ra,sb->ijab', _eri(mf), co, co, cv, cv, optimize=True)
    A = -hyb * ijab.transpose(2, 0, 3, 1).reshape(nv * no, nv * no)         # rows (a, i), columns (b, j)
    A[np.diag_indices(nv * no)] += (ev[:, None] - eo[None, :]).ravel()
    e, v = np.linalg.eigh(A)
    return e, v.T.reshape(-1, nv, no)


# ------------------------------------------------------------------ the gradient
def _kxc_matrix(xa, s, occ, vir):
    """<a i| w fxc |b j> over the vo pairs of both working spins (rows and columns: spin "a" then
    spin "b", each (virtual, occupied) row-major): the XC part of the Z-vector matrix, from the MO
    values on the grid.  The response of a symmetrised unit rotation a <- i has
    rho1 = psi_a psi_i and grad rho1 = grad(psi_a psi_i), and <a|V^resp|i> contracts wv with the same."""
    nc = 4 if xa.gga else 1
    ao = xa.ao10[:nc]
    rr = []
    for t in range(2):
        po, pv = ao @ occ[t], ao @ vir[t]                                    # (nc, G, nocc), (nc, G, nvir)
        r = np.einsum('ga,gi->gai', pv[0], po[0])[None]
        if xa.gga:
            r = np.concatenate([r, np.einsum('kga,gi->kgai', pv[1:], po[0]) + np.einsum('ga,kgi->kgai', pv[0], po[1:])])
        rr.append(r.reshape(nc, r.shape[1], -1))
    blocks = [[np.einsum('kgp,klg,lgq->pq', rr[t], xa.w * xa.fxc[s[t], :, s[u]], rr[u], optimize=True)
               for u in range(2)] for t in range(2)]
    return np.block(blocks)


def sf_ks_grad(mf, x, isf, ip=None, xa=None, hyb=None, with_fxc=True, mcache=None):
    """(d(E_SCF + omega)/dR (natm, 3), S, parts) of the collinear spin-flip TDA state with amplitude
    x (nvir_f, nocc_i); isf = +1 exchanges the spin labels.  ``xa``: the XC arrays (default: those of
    the mean field), ``hyb``: the exchange fraction (default: the mean field's); ``with_fxc`` False
    drops every term the second functional derivative enters.  ``mcache``: a dict that keeps the
    Z-vector matrix, which does not depend on the state, between calls on the same mean field.
    parts: xc (the XC nuclear-derivative part), xc_fxc (its G_xc[wv; D0] term), sum_atoms."""
    mol = mf.mol
    ip = R.deriv_eri(mol) if ip is None else ip
    xa = xc_arrays(mf) if xa is None else xa
    if not with_fxc:
        xa = xa._replace(fxc=np.zeros_like(xa.fxc))
    hyb = float(mf.hyb) if hyb is None else float(hyb)
    eri = _eri(mf)
    s = (0, 1) if isf == -1 else (1, 0)

    def order(pair):             # working labels <-> alpha, beta (s is its own inverse)
        return np.asarray([pair[s[0]], pair[s[1]]])

    def fx(pair):                # V^resp in the working labels, with its S
        v, _, sv, _ = vresp_xc(xa, order(pair))
        return order(v), order(sv)
    C = [mf.mo_coeff[t] for t in s]
    occ = [mf.mo_occ[t] > 0 for t in s]
    f_ao = mf.get_hcore()[None] + np.asarray(mf._veff)
    F = [C[t].T @ f_ao[s[t]] @ C[t] for t in range(2)]
    oa, va, ob, vb = C[0][:, occ[0]], C[0][:, ~occ[0]], C[1][:, occ[1]], C[1][:, ~occ[1]]
    na, nb = oa.shape[1], ob.shape[1]
    x = x / np.linalg.norm(x)
    ta, tb = -x.T @ x, x @ x.T
    dta, dtb = oa @ ta @ oa.T, vb @ tb @ vb.T
    dta, dtb = (dta + dta.T) / 2, (dtb + dtb.T) / 2
    dx = vb @ x @ oa.T
    xs, xan = (dx + dx.T) / 2, (dx - dx.T) / 2
    vj, vk = R._jk(eri, [dta, dtb, xs, xan])
    vk = hyb * vk
    kx = C[1].T @ (vk[2] + vk[3]) @ C[0]
    ft, _ = fx((dta, dtb))
    ga, gb = vj[0] + vj[1] - vk[0] + ft[0], vj[0] + vj[1] - vk[1] + ft[1]
    ra = 2 * (va.T @ ga @ oa + F[0][na:, :na] @ ta.T - kx[nb:, na:].T @ x)
    rb = 2 * (vb.T @ gb @ ob - tb @ F[1][:nb, nb:].T + x @ kx[:nb, :na].T)
    nva, nvb = va.shape[1], vb.shape[1]
    dim = nva * na + nvb * nb

    def resp(pair):              # J - hyb K + V^resp of a symmetric pair
        j, k = R._jk(eri, pair)
        return (j[0] + j[1])[None] - hyb * k + fx(pair)[0]

    def apply(z):                # the J / K and orbital-energy part of the Z-vector operator
        za, zb = z[:nva * na].reshape(nva, na), z[nva * na:].reshape(nvb, nb)
        da, db = va @ za @ oa.T, vb @ zb @ ob.T
        j, k = R._jk(eri, ((da + da.T) / 2, (db + db.T) / 2))
        v = 2 * ((j[0] + j[1])[None] - hyb * k)
        ra_ = va.T @ v[0] @ oa + F[0][na:, na:].T @ za - za @ F[0][:na, :na].T
        rb_ = vb.T @ v[1] @ ob + F[1][nb:, nb:].T @ zb - zb @ F[1][:nb, :nb].T
        return np.hstack((ra_.ravel(), rb_.ravel()))
    key = (isf, bool(with_fxc))
    if mcache is not None and key in mcache:
        M = mcache[key]
    else:
        M = np.stack([apply(e) for e in np.eye(dim)], axis=1) + 2.0 * _kxc_matrix(xa, s, (oa, ob), (va, vb))
        if mcache is not None:
            mcache[key] = M
    z = np.linalg.solve(M, -np.hstack((ra.ravel(), rb.ravel())))
    za, zb = z[:nva * na].reshape(nva, na), z[nva * na:].reshape(nvb, nb)
    zao = [va @ za @ oa.T, vb @ zb @ ob.T]
    zs = [(m + m.T) / 2 for m in zao]
    gz = resp(zs)
    wa, wb = np.zeros_like(F[0]), np.zeros_like(F[1])
    wa[:na, :na] = F[0][:na, :na] + oa.T @ (ga + gz[0]) @ oa + ta @ F[0][:na, :na] - x.T @ kx[nb:, :na]
    wb[:nb, :nb] = F[1][:nb, :nb] + ob.T @ (gb + gz[1]) @ ob
    wb[nb:, nb:] = tb @ F[1][nb:, nb:].T - x @ kx[nb:, :na].T
    wa[na:, :na] = za @ F[0][:na, :na].T
    wb[nb:, :nb] = zb @ F[1][:nb, :nb].T - 2 * x @ kx[:nb, :na].T
    W = C[0] @ wa @ C[0].T + C[1] @ wb @ C[1].T
    d0a, d0b = oa @ oa.T, ob @ ob.T
    pa, pb = zs[0] + dta, zs[1] + dtb
    h = hyb
    pairs = [(1, 0, d0a + d0b, d0a + d0b), (0, -h, d0a, d0a), (0, -h, d0b, d0b),
             (1, 0, d0a + d0b, pa + pb), (0, -h, d0a, pa), (0, -h, d0b, pb),
             (1, 0, pa + pb, d0a + d0b), (0, -h, pa, d0a), (0, -h, pb, d0b),
             (0, -2 * h, xs, xs)]
    g1, g2, gn = R._de_1e(mol, d0a + d0b + pa + pb, W), R._de_2e(mol, ip, pairs), R._nuc(mol)
    on = mol.ao_atom()
    vka = -np.einsum('xijkl,jk->xil', ip, xan, optimize=True)
    per_ao = -2 * h * np.einsum('xpq,pq->xp', vka, xan - xan.T)
    g2 = g2 + np.stack([per_ao[:, on == A].sum(axis=1) for A in range(mol.natm)])
    # XC: G_xc[w vxc[rho0]; P] + G_xc[wv[T + Z^S]; D0], everything in the order alpha, beta
    d0, tz = order((d0a, d0b)), order((pa, pb))
    gx1, s1 = gxc(mol, xa, xa.h0, d0 + tz)
    wv = vresp_xc(xa, tz)[1]
    gx2, s2 = gxc(mol, xa, wv, d0)
    g = g1 + g2 + gn + gx1 + gx2
    S = float(np.abs(g1).sum() + np.abs(g2).sum() + np.abs(gn).sum() + s1 + s2)
    return g, S, dict(xc=gx1 + gx2, xc_fxc=gx2, sum_atoms=g.sum(axis=0), omega_rhs=(ra, rb))
