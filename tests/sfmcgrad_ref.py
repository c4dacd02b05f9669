"""NumPy restatement of the multicollinear spin-flip TDA gradient on a UKS reference, on a grid held
fixed in space (TEST INFRASTRUCTURE ONLY; not a test file).

``tests/sfksgrad_ref.py`` (the collinear kernel) with the three changes of DESIGN section 18, in a
formulation the device code does not share:

* the explicit tensor kxc_sf(x, y, s, k, g) = d fxc_sf(x, y, g) / d rho0_s(k, g): the Hessian of the
  energy density in the spin variables at every sample, row by row, summed over the samples, and one host
  autograd pass per (x, y) pair; wv2 is its ``einsum`` with rho1 twice, as the reference contracts its
  ``kxc_sf``;
* A = the collinear A + 2 <ia| w fxc_sf |jb> from the MO values on the grid;
* plain ``einsum`` for rho1, wv1 and the potentials, a dense solve of the Z-vector equations.

Everything XC stays in the order alpha, beta; S (absolute-value sums) comes with every summed quantity.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import grad_ref as R
import sfksgrad_ref as SK
from xtddft_amd.qc import xc as _xc

RHO_SHIFT = 1e-11      # SF_TDA.py:969
# fsf (nk, nk, G) un-weighted; kxc (nk, nk, 2, nk, G) or None
MCArrays = namedtuple("MCArrays", "fsf kxc")


def rho_of(ao, dms, gga):
    """(2, nk, G) spin densities of symmetric density matrices on AO values ao (>= nk, G, nao)."""
    dms = np.asarray(dms)
    c = np.einsum('gn,snm->sgm', ao[0], dms)
    rho = np.zeros((2, 4 if gga else 1, ao.shape[1]))
    rho[:, 0] = np.einsum('gm,sgm->sg', ao[0], c)
    if gga:
        rho[:, 1:] = 2.0 * np.einsum('kgm,sgm->skg', ao[1:4], c)
    return rho


def mc_arrays(xc, rho0, samples, with_grad=True, device="cpu"):
    """fxc_sf (nk, nk, G) and, ``with_grad``, kxc_sf (nk, nk, 2, nk, G) at spin densities rho0 (2, nk, G).
    ``device``: where the autograd runs; the host by default (one thread: the graphs are element-wise).
    The GPU tests, whose grid has 33 734 points, pass "cuda" for the whole grid, where the host takes
    about a minute per functional, and assert that array equal to the host one on a subsample of the
    points (``tests/test_gpu_sfmcgrad.py`` ``_mc_arrays``)."""
    import torch
    if str(device) != "cpu":
        return _mc_arrays(torch, xc, rho0, samples, with_grad, torch.device(device))
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _mc_arrays(torch, xc, rho0, samples, with_grad, torch.device("cpu"))
    finally:
        torch.set_num_threads(nthreads)


def _mc_arrays(torch, xc, rho0, samples, with_grad, dev):
    comps, _, xctype = _xc.parse_xc(xc)
    rho0 = np.asarray(rho0, dtype=np.float64)
    nk, G = rho0.shape[1], rho0.shape[2]
    t, wt = np.polynomial.legendre.leggauss(int(samples))
    t, wt = 0.5 * t + 0.5, 0.5 * wt
    r0 = torch.tensor(rho0, dtype=torch.float64, device=dev, requires_grad=True)
    tt = r0[0] + r0[1] + RHO_SHIFT
    ss = r0[0] - r0[1] + RHO_SHIFT
    # every sample of every point in one graph: columns (sample, point)
    tk = torch.as_tensor(t, dtype=torch.float64, device=dev)
    wcol = torch.as_tensor(wt, dtype=torch.float64, device=dev).repeat_interleave(G)
    sk = ss[:, None, :] * tk[None, :, None]
    ua, ub = (0.5 * (tt[:, None, :] + sk)).reshape(nk, -1), (0.5 * (tt[:, None, :] - sk)).reshape(nk, -1)
    keep = torch.nonzero((ua[0] + ub[0]).detach() > _xc.DENS_THRESHOLD).squeeze(1)
    F = torch.zeros((nk, nk, G), dtype=torch.float64, device=dev)
    if keep.numel():
        x = torch.stack([ua, ub])[:, :, keep]                            # (2, nk, n)
        ra, rb = torch.clamp(x[0, 0], min=1e-30), torch.clamp(x[1, 0], min=1e-30)
        if nk == 4:
            saa, sab, sbb = (x[0, 1:] * x[0, 1:]).sum(0), (x[0, 1:] * x[1, 1:]).sum(0), (x[1, 1:] * x[1, 1:]).sum(0)
        else:
            saa = sab = sbb = torch.zeros_like(ra)
        on = ((x[0, 0] > _xc.DENS_THRESHOLD).to(torch.float64).detach(),
              (x[1, 0] > _xc.DENS_THRESHOLD).to(torch.float64).detach())
        eps = _xc._energy_density(comps, ra, rb, saa, sab, sbb, None, None, torch, on)
        g = torch.autograd.grad(eps.sum(), x, create_graph=True)[0]
        gs = 0.5 * (g[0] - g[1])                                         # d eps / d s_k, s = rho_a - rho_b
        H = torch.stack([torch.autograd.grad(gs[k].sum(), x, create_graph=True)[0] for k in range(nk)])
        fss = 0.5 * (H[:, 0] - H[:, 1])                                  # d2 eps / d s_k d s_k', (k, k', n)
        full = torch.zeros((nk, nk, len(t) * G), dtype=torch.float64, device=dev).index_add(2, keep, fss * wcol[keep])
        F = full.reshape(nk, nk, len(t), G).sum(2)
    F = 0.5 * (F + F.transpose(0, 1))
    kxc = None
    if with_grad:
        kxc = np.zeros((nk, nk, 2, nk, G))
        if F.requires_grad:
            # one backward pass per (x, y) pair, x <= y, the pairs batched (they share the graph)
            pairs = [(a, b) for a in range(nk) for b in range(a, nk)]
            sel = torch.zeros((len(pairs), nk, nk), dtype=torch.float64, device=dev)
            for n, (a, b) in enumerate(pairs):
                sel[n, a, b] = 1.0
            d = torch.autograd.grad(F.sum(2), r0, grad_outputs=sel, is_grads_batched=True)[0].cpu().numpy()
            for n, (a, b) in enumerate(pairs):
                kxc[a, b] = kxc[b, a] = d[n]
    return MCArrays(F.detach().cpu().numpy(), kxc)


def mc_arrays_of(mf, xa, samples, with_grad=True, device="cpu"):
    return mc_arrays(mf.xc, rho_of(xa.ao10, SK._d0(mf), xa.gga), samples, with_grad, device)


def zero_mc_arrays(xa):
    nk, G = (4 if xa.gga else 1), xa.w.size
    return MCArrays(np.zeros((nk, nk, G)), np.zeros((nk, nk, 2, nk, G)))


def sf_weights(xa, mc, x_s):
    """(rho1 (nk, G), wv1 (4, G), wv2 (2, 4, G) or None, S_wv1) of the symmetric transition density."""
    nk = 4 if xa.gga else 1
    ao = xa.ao10
    c = ao[0] @ x_s
    sc = np.abs(ao[0]) @ np.abs(x_s)
    rho1, s_rho = np.zeros((nk, xa.w.size)), np.zeros((nk, xa.w.size))
    rho1[0], s_rho[0] = np.einsum('gm,gm->g', ao[0], c), np.einsum('gm,gm->g', np.abs(ao[0]), sc)
    if xa.gga:
        rho1[1:] = 2.0 * np.einsum('kgm,gm->kg', ao[1:4], c)
        s_rho[1:] = 2.0 * np.einsum('kgm,gm->kg', np.abs(ao[1:4]), sc)
    wv1, s_wv1 = np.zeros((4, xa.w.size)), np.zeros((4, xa.w.size))
    wv1[:nk] = 2.0 * xa.w * np.einsum('klg,lg->kg', mc.fsf, rho1)
    s_wv1[:nk] = 2.0 * np.abs(xa.w) * np.einsum('klg,lg->kg', np.abs(mc.fsf), s_rho)
    wv2 = None
    if mc.kxc is not None:
        wv2 = np.zeros((2, 4, xa.w.size))
        wv2[:, :nk] = 2.0 * xa.w * np.einsum('xg,xyskg,yg->skg', rho1, mc.kxc, rho1)
    return rho1, wv1, wv2, s_wv1


def potential(xa, wv):
    """(V (nao, nao), S) of the weights wv (4, G), unhalved: phi^T b (+ its transpose for GGA)."""
    ao = xa.ao10
    if xa.gga:
        b = 0.5 * wv[0][:, None] * ao[0] + np.einsum('kg,kgm->gm', wv[1:4], ao[1:4])
        sb = 0.5 * np.abs(wv[0])[:, None] * np.abs(ao[0]) + np.einsum('kg,kgm->gm', np.abs(wv[1:4]), np.abs(ao[1:4]))
    else:
        b, sb = wv[0][:, None] * ao[0], np.abs(wv[0])[:, None] * np.abs(ao[0])
    v, sv = ao[0].T @ b, np.abs(ao[0]).T @ sb
    return (v + v.T, sv + sv.T) if xa.gga else (v, sv)


def _spaces(mf, isf):
    s = (0, 1) if isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    eo = mf.mo_energy[s[0]][mf.mo_occ[s[0]] > 0]
    ev = mf.mo_energy[s[1]][mf.mo_occ[s[1]] == 0]
    return co, cv, eo, ev


def sf_mc_amat(mf, isf, xa, mc, hyb=None):
    """The multicollinear spin-flip A matrix, rows and columns (a, i) row-major: the collinear one of
    ``sfksgrad_ref.sf_states`` plus 2 <a i| w fxc_sf |b j> from the MO values on the grid."""
    hyb = float(mf.hyb) if hyb is None else hyb
    co, cv, eo, ev = _spaces(mf, isf)
    no, nv = co.shape[1], cv.shape[1]
    ijab = np.einsum('pqrs,pi,qj,ra,sb->ijab', SK._eri(mf), co, co, cv, cv, optimize=True)
    A = -hyb * ijab.transpose(2, 0, 3, 1).reshape(nv * no, nv * no)
    A[np.diag_indices(nv * no)] += (ev[:, None] - eo[None, :]).ravel()
    nk = 4 if xa.gga else 1
    ao = xa.ao10[:nk]
    po, pv = ao @ co, ao @ cv
    r = np.einsum('ga,gi->gai', pv[0], po[0])[None]
    if xa.gga:
        r = np.concatenate([r, np.einsum('kga,gi->kgai', pv[1:], po[0]) + np.einsum('ga,kgi->kgai', pv[0], po[1:])])
    r = r.reshape(nk, r.shape[1], -1)
    return A + 2.0 * np.einsum('kgp,klg,lgq->pq', r, xa.w * mc.fsf, r, optimize=True)


def sf_mc_states(mf, isf, xa, mc, hyb=None):
    """(omega ascending, x (root, nvir_f, nocc_i)) of ``sf_mc_amat``."""
    co, cv, _, _ = _spaces(mf, isf)
    e, v = np.linalg.eigh(sf_mc_amat(mf, isf, xa, mc, hyb))
    return e, v.T.reshape(-1, cv.shape[1], co.shape[1])


def sf_mc_grad(mf, x, isf, ip=None, xa=None, mc=None, hyb=None, mcache=None):
    """(d(E_SCF + omega)/dR (natm, 3), S, parts) of the multicollinear spin-flip TDA state with amplitude
    x (nvir_f, nocc_i): ``sfksgrad_ref.sf_ks_grad`` with hyb K[X] - V_sf in the coupling matrix, V^k
    next to f^xc[T], and G_xc[wv2; D0] + 2 G_xc[wv1; X_S] in the XC nuclear-derivative part.
    parts: xc, xc_sf (2 G_xc[wv1; X_S]), xc_k (G_xc[wv2; D0]), sum_atoms."""
    mol = mf.mol
    ip = R.deriv_eri(mol) if ip is None else ip
    xa = SK.xc_arrays(mf) if xa is None else xa
    hyb = float(mf.hyb) if hyb is None else float(hyb)
    eri = SK._eri(mf)
    s = (0, 1) if isf == -1 else (1, 0)

    def order(pair):
        return np.asarray([pair[s[0]], pair[s[1]]])

    def fx(pair):
        v, _, sv, _ = SK.vresp_xc(xa, order(pair))
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
    # the multicollinear kernel: V_sf next to hyb K[X], V^k next to f^xc[T]
    _, wv1, wv2, _ = sf_weights(xa, mc, xs)
    vsf, s_vsf = potential(xa, wv1)
    vkk = order([potential(xa, wv2[t])[0] for t in range(2)])
    kx = C[1].T @ (vk[2] + vk[3] - vsf) @ C[0]
    ft, _ = fx((dta, dtb))
    ga, gb = vj[0] + vj[1] - vk[0] + ft[0] + vkk[0], vj[0] + vj[1] - vk[1] + ft[1] + vkk[1]
    ra = 2 * (va.T @ ga @ oa + F[0][na:, :na] @ ta.T - kx[nb:, na:].T @ x)
    rb = 2 * (vb.T @ gb @ ob - tb @ F[1][:nb, nb:].T + x @ kx[:nb, :na].T)
    nva, nvb = va.shape[1], vb.shape[1]
    dim = nva * na + nvb * nb

    def resp(pair):
        j, k = R._jk(eri, pair)
        return (j[0] + j[1])[None] - hyb * k + fx(pair)[0]

    def apply(z):
        za, zb = z[:nva * na].reshape(nva, na), z[nva * na:].reshape(nvb, nb)
        da, db = va @ za @ oa.T, vb @ zb @ ob.T
        j, k = R._jk(eri, ((da + da.T) / 2, (db + db.T) / 2))
        v = 2 * ((j[0] + j[1])[None] - hyb * k)
        ra_ = va.T @ v[0] @ oa + F[0][na:, na:].T @ za - za @ F[0][:na, :na].T
        rb_ = vb.T @ v[1] @ ob + F[1][nb:, nb:].T @ zb - zb @ F[1][:nb, :nb].T
        return np.hstack((ra_.ravel(), rb_.ravel()))
    if mcache is not None and isf in mcache:
        M = mcache[isf]
    else:
        M = np.stack([apply(e) for e in np.eye(dim)], axis=1) + 2.0 * SK._kxc_matrix(xa, s, (oa, ob), (va, vb))
        if mcache is not None:
            mcache[isf] = M
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
    # XC: G_xc[w vxc; P] + G_xc[wv[T + Z^S]; D0] + G_xc[wv2; D0] + 2 G_xc[wv1; X_S]
    d0, tz = order((d0a, d0b)), order((pa, pb))
    gx1, s1 = SK.gxc(mol, xa, xa.h0, d0 + tz)
    gx2, s2 = SK.gxc(mol, xa, SK.vresp_xc(xa, tz)[1], d0)
    gxk, sk = SK.gxc(mol, xa, wv2, d0)
    gxs, ssf = SK.gxc(mol, xa, np.asarray([2.0 * wv1, np.zeros_like(wv1)]), np.asarray([xs, np.zeros_like(xs)]))
    g = g1 + g2 + gn + gx1 + gx2 + gxk + gxs
    S = float(np.abs(g1).sum() + np.abs(g2).sum() + np.abs(gn).sum() + s1 + s2 + sk + ssf)
    return g, S, dict(xc=gx1 + gx2 + gxk + gxs, xc_sf=gxs, xc_k=gxk, sum_atoms=g.sum(axis=0), s_vsf=s_vsf)
