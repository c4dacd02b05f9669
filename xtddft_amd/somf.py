"""The sf-X2C / soDKH1 spin-orbit mean-field operator Vso (the reference's
``x2c_hamiltonian/sfX2C_soDKH1.py``; Li, Xiao, Liu, JCP 137, 154114 (2012)): the input of
``soc.SI_driver`` that test_SOCSI.py:105-108 builds with

    Vso_ao = get_soDKH1_somf(mf, mol, c, iop='x2c', include_mf2e=True)
    Vso_mo = vso_mo(mf, Vso_ao)

The nao-sized X2C algebra (``sfx2c1e``, ``get_p``, ``get_hso1e``, ``finalize_fso2e``) runs on
the host once per molecule, like the SCF's own eigenproblems.  The O(N^4) part -- the
two-electron spin-orbit integrals K^l = eps_lmn (d_m mu  nu | d_n ka  la) contracted with the
spin-averaged densities -- runs on the GPU (``qc.dints.somf_g_device``, kernel
``xt_hint_cart``); ``device=None`` takes the host restatement ``somf_g_host`` (small molecules:
it stores K).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

LIGHT_SPEED = 137.0359895      # test_SOCSI.py:105


# ---------------------------------------------------------------- X2C algebra
def _inv_sqrt(s):
    e, v = scipy.linalg.eigh(s)
    return (v / np.sqrt(e)) @ v.T


def sfx2c1e(t, v, w, s, c):
    """(x, rp, h1e) of the spin-free one-electron X2C (sfX2C_soDKH1.py:150-183): the modified
    Dirac equation  [[V, T], [T, W / 4c^2 - T]] C = [[S, 0], [0, T / 2c^2]] C e  in the
    primitive basis; x = C_S C_L^-1 over the positive-energy half, the renormalisation
    rp = S^-1/2 (S^-1/2 S~ S^-1/2)^-1/2 S^1/2 with S~ = S + x^T (T / 2c^2) x, and
    h1e = rp^T (V + T x + x^T T + x^T (W / 4c^2 - T) x) rp."""
    n = s.shape[0]
    h = np.zeros((2 * n, 2 * n))
    m = np.zeros((2 * n, 2 * n))
    wss = w * (0.25 / c ** 2) - t
    h[:n, :n], h[:n, n:], h[n:, :n], h[n:, n:] = v, t, t, wss
    m[:n, :n], m[n:, n:] = s, t * (0.5 / c ** 2)
    _, a = scipy.linalg.eigh(h, m)
    cl, cs = a[:n, n:], a[n:, n:]
    x = cs @ cl.T @ np.linalg.inv(cl @ cl.T)
    st = s + x.T @ m[n:, n:] @ x
    sih = _inv_sqrt(s)
    sh = np.linalg.inv(sih)
    rp = sih @ _inv_sqrt(sih @ st @ sih) @ sh
    l1e = v + t @ x + x.T @ t + x.T @ wss @ x
    return x, rp, rp.T @ l1e @ rp


def get_p(dm, x, rp):
    """Spin-averaged densities of the large / small components (:185-200)."""
    pLL = rp @ dm @ rp.T
    return pLL, pLL @ x.T, x @ pLL @ x.T


def get_hso1e(wso, x, rp):
    """rp^T x^T W^l x rp per component (:241-255)."""
    xr = x @ rp
    return np.stack([xr.T @ w @ xr for w in wso])


def finalize_fso2e(gsoLL, gsoLS, gsoSS, x, rp):
    """rp^T [G_LL + G_LS x - x^T G_LS^T + x^T G_SS x] rp per component (:401-410)."""
    return np.stack([rp.T @ (gll + gls @ x - x.T @ gls.T + x.T @ gss @ x) @ rp
                     for gll, gls, gss in zip(gsoLL, gsoLS, gsoSS)])


# ---------------------------------------------------------------- host restatement of the SOMF
def kint_host(mol, use_1c: bool = False):
    """K^l[mu, nu, ka, la] = eps_lmn (d_m mu  nu | d_n ka  la) over normalised spherical AOs,
    (3, nao, nao, nao, nao), on the host (get_kint, :218-239); ``use_1c``: the quartets with all
    four shells on one atom, zero elsewhere."""
    from .qc.gto import _sph_transform
    from .qc.ints import DerivPair, cross3, eri_quartet_kets
    sh, loc, n = mol.shells, mol.ao_loc, mol.nao
    T = [_sph_transform(s.l) for s in sh]
    pairs = {(i, j): DerivPair(sh[i], sh[j]) for i in range(len(sh)) for j in range(len(sh))
             if not use_1c or sh[i].atom == sh[j].atom}
    K = np.zeros((3, n, n, n, n))
    classes = {}                     # kets of one class are evaluated in one pass per bra
    for key, ket in pairs.items():
        classes.setdefault((ket.L, ket.Eab.shape), []).append(key)
    for (i, j), bra in pairs.items():
        for keys in classes.values():
            if use_1c:
                keys = [kl for kl in keys if sh[kl[0]].atom == sh[i].atom]
                if not keys:
                    continue
            g = eri_quartet_kets(bra, [pairs[kl] for kl in keys])[:, :, 0, :, 0]      # (K, 3 nab, 3 ncd)
            for (k, l), gk in zip(keys, g):
                gk = gk.reshape(3, sh[i].ncart, sh[j].ncart, 3, sh[k].ncart, sh[l].ncart)
                blk = np.einsum('ai,bj,xijkl,ck,dl->xabcd', T[i], T[j], cross3(gk, 0, 3), T[k], T[l], optimize=True)
                K[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1], loc[k]:loc[k + 1], loc[l]:loc[l + 1]] = blk
    nrm = mol._norm
    K *= (nrm[:, None, None, None] * nrm[None, :, None, None] * nrm[None, None, :, None] * nrm[None, None, None, :])
    return K


def somf_g_host(mol, pLL, pLS, pSS, use_1c: bool = True, kint=None):
    """(gsoLL, gsoLS, gsoSS), each (3, nao, nao): the six contractions of get_fso2e (:257-282)
    with the stored K of ``kint_host`` (index names as in qc.dints.somf_g_device)."""
    K = kint_host(mol, use_1c) if kint is None else kint
    gLL = -2.0 * np.einsum('xmnkl,mk->xnl', K, pSS)
    gLS = -np.einsum('xmnkl,nk->xml', K, pLS) - np.einsum('xmnkl,mk->xnl', K, pLS)
    gSS = (-2.0 * np.einsum('xmnkl,lk->xmn', K, pLL + pLL.T) + 2.0 * np.einsum('xmnkl,nl->xmk', K, pLL))
    return gLL, gLS, gSS


# ---------------------------------------------------------------- the sf-X2C mean field
class X2C:
    """``mf.with_x2c``: the primitive basis and the spin-free X2C core Hamiltonian in the
    contracted one."""

    def __init__(self, mol, c: float = LIGHT_SPEED):
        self.mol, self.c = mol, float(c)
        self._xmol = None

    def get_xmol(self, mol=None):
        from .qc.gto import get_xmol
        if mol is not None and mol is not self.mol:
            return get_xmol(mol)
        if self._xmol is None:
            self._xmol = get_xmol(self.mol)
        return self._xmol

    def get_hcore(self, device=None):
        xmol, cc = self.get_xmol()
        h1e = sfx2c1e(*_tvws(xmol, device), self.c)[2]
        return cc.T @ h1e @ cc


def _tvws(xmol, device):
    return (xmol.intor("int1e_kin"), xmol.intor("int1e_nuc", device=device),
            xmol.intor("int1e_pnucp", device=device), xmol.intor("int1e_ovlp"))


# ---------------------------------------------------------------- the public function
def get_soDKH1_somf(myhf, mol, c: float = LIGHT_SPEED, iop: str = "x2c", include_mf2e=True, mf2e_impl="auto",
                    nproc: int = 1, use_1c: bool = True, debug: bool = False, device=0, dm=None,
                    chunk_pairs=None, timings=None):
    """Vso in the AO basis, (3, nao, nao), real antisymmetric (sfX2C_soDKH1.py:692-852):
    a4 [hso1e + fso2e] with a4 = 1 / 4c^2, contracted back with ``contr_coeff`` when ``myhf``
    has ``with_x2c`` (the primitive basis; otherwise ``mol`` itself).  iop 'x2c': X and R from
    ``sfx2c1e``; 'bp': X = R = 1 (Breit-Pauli).  ``mf2e_impl`` and ``nproc`` are accepted for
    signature compatibility and ignored: there is one implementation.  ``device``: the GPU
    (None: the host restatement).  ``dm`` overrides ``myhf.make_rdm1()`` (a total density or
    an (alpha, beta) pair); ``chunk_pairs`` overrides the ket chunk of the device contraction."""
    if hasattr(myhf, "with_x2c") and myhf.with_x2c is not None:
        xmol, contr = myhf.with_x2c.get_xmol(mol)
    else:
        xmol, contr = mol, np.eye(mol.nao)
    nb = contr.shape[0]
    if iop == "x2c":
        x, rp, _ = sfx2c1e(*_tvws(xmol, device), c)
    elif iop == "bp":
        x, rp = np.eye(nb), np.eye(nb)
    else:
        raise ValueError(f"iop={iop!r} not in ('x2c', 'bp')")
    dm = np.asarray(myhf.make_rdm1() if dm is None else dm)
    dm = 0.5 * (dm[0] + dm[1]) if dm.ndim == 3 else 0.5 * dm      # occupations 1, 1/2, 0
    dm = contr @ dm @ contr.T
    pLL, pLS, pSS = get_p(dm, x, rp)
    wso = xmol.intor("int1e_wso", device=device)
    a4 = 0.25 / c ** 2
    hso1e = get_hso1e(wso, x, rp)
    vso = a4 * hso1e
    fso2e = None
    if include_mf2e:
        if device is None:
            g = somf_g_host(xmol, pLL, pLS, pSS, use_1c)
        else:
            from .qc.dints import somf_g_device
            g = somf_g_device(xmol, pLL, pLS, pSS, use_1c, device, chunk_pairs, timings)
        fso2e = finalize_fso2e(*g, x, rp)
        vso = vso + a4 * fso2e
    if debug:
        for ic in range(3):
            for name, mat in (("hso1e", hso1e[ic]), ("fso2e", None if fso2e is None else fso2e[ic])):
                if mat is not None:
                    print(f"{ic} {name} norm={np.linalg.norm(mat):.12e}, "
                          f"Norm(tmp+tmp.T)={np.linalg.norm(mat + mat.T):.12e}")
    return np.stack([contr.T @ v @ contr for v in vso])


def vso_mo(mf, vso_ao):
    """Vso in the MO basis of ``mf`` (test_SOCSI.py:108): C^T Vso^l C; ROKS orbitals."""
    c = np.asarray(mf.mo_coeff)
    if c.ndim != 2:
        raise ValueError("vso_mo needs one set of orbitals (ROHF / ROKS)")
    return np.einsum('nij,ik,jl->nkl', vso_ao, c, c, optimize=True)
