"""Analytic nuclear gradients: the pieces every gradient shares, and the UHF ground state.

* one-electron derivatives as PySCF's ``grad.rhf`` / ``grad.uhf`` return them (the reference's
  ``grad_jp/grad/usfcis.py:193-195`` reads them from ``mf.nuc_grad_method()``):
  ``get_ovlp(mol)`` = -<nabla mu|nu> (3, nao, nao), ``hcore_generator(mol)(ia)`` and
  ``grad_nuc(mol)``; built on the host from ``ShellPair.deriv1``, ``ints.kinetic_deriv1`` and
  the Hermite tables of ``DerivPair`` (nao^2 natm objects);
* ``grad_jk_device`` -- the contraction of the first-derivative ERIs with a two-particle
  density through the library kernel ``xt_grad_jk`` (``csrc/xt_grad.hip``): every
  ``get_jk`` / ``get_k`` gradient term of the reference in one call,

      g[A, m] = sum_{a on A} sum_{bcd} (d_m a  b|c d) sum_t wj_t P_t[a,b] Q_t[c,d] + wk_t P_t[a,c] Q_t[b,d];

  PySCF's ``vj[x,i,j] = -(d_x i j|k l) D[l,k]``, ``vk[x,i,l] = -(d_x i j|k l) D[j,k]`` and
  ``de_A += sum_{p on A, q} v[x,p,q] (D'[p,q] + D'[q,p])`` are the terms
  (wj, wk, P, Q) = (-1, 0, D' + D'^T, D^T) and (0, -1, D' + D'^T, D) (``jk_terms``);
* ``solve_zvector`` -- the UCPHF Z-vector equations (usfcis.py:127-150) by a host-driven
  preconditioned GMRES whose response J / K come from ``DeviceEngine.get_jk``;
* ``Gradients`` -- ``UHF.nuc_grad_method()``: the T = Z = X = 0 subset of the excited-state
  formula with W the energy-weighted density.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np

from .. import _capi
from .gto import _sph_transform
from .ints import DerivPair, hermite_r, kinetic_deriv1

MAX_TERMS = 8
MAX_CHOL_TOL = 1e-10     # loosest ERI Cholesky tolerance a gradient accepts (check_gradient_mf)
# bra / ket order bounds of the kernel's three dispatch buckets (s p | d | f shells)
BRA_BOUNDS = (4, 6, 8)
KET_BOUNDS = (2, 4, 6)


# ------------------------------------------------------------------ one-electron derivatives
def _to_sph(mol, i, j, blk):
    """Cartesian (3, nca, ncb) block of shells i, j -> normalised spherical (3, nsa, nsb)."""
    Ti, Tj = _sph_transform(mol.shells[i].l), _sph_transform(mol.shells[j].l)
    ni = mol._norm[mol.ao_loc[i]:mol.ao_loc[i + 1]]
    nj = mol._norm[mol.ao_loc[j]:mol.ao_loc[j + 1]]
    return np.einsum('mi,dij,nj->dmn', Ti, blk, Tj) * ni[None, :, None] * nj[None, None, :]


def get_ovlp(mol):
    """-<nabla mu|nu>, (3, nao, nao): PySCF ``grad.rhf.get_ovlp`` (-int1e_ipovlp)."""
    return -mol.intor("int1e_ipovlp")


def ipkin(mol):
    """<nabla mu| -1/2 nabla^2 |nu>, (3, nao, nao): PySCF ``int1e_ipkin``."""
    n = mol.nao
    out = np.zeros((3, n, n))
    loc = mol.ao_loc
    for i, si in enumerate(mol.shells):
        for j, sj in enumerate(mol.shells):
            out[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = _to_sph(mol, i, j, kinetic_deriv1(si, sj))
    return out


def iprinv_atoms(mol):
    """(natm, 3, nao, nao): -Z_C <nabla mu| 1/|r - R_C| |nu> for every nucleus C (PySCF
    ``int1e_iprinv`` at each nucleus times -Z_C; their sum over C is ``int1e_ipnuc``).  The tables
    of ``DerivPair`` hold the derivative with respect to the centre of mu, the negative of nabla."""
    n, natm = mol.nao, mol.natm
    out = np.zeros((natm, 3, n, n))
    loc = mol.ao_loc
    Z, Rc = mol._charges, mol.atom_coords()
    for i, si in enumerate(mol.shells):
        for j, sj in enumerate(mol.shells):
            dp = DerivPair(si, sj)
            d = dp.P[:, None, :] - Rc[None, :, :]                                  # (q, C, 3)
            R = hermite_r(dp.L, dp.p[:, None], d[..., 0], d[..., 1], d[..., 2])     # (t, q, C)
            v = np.einsum('atq,tqC->Ca', dp.Eab[:, 0], R * (2.0 * np.pi / dp.p)[None, :, None]) * Z[:, None]
            for c in range(natm):
                out[c][:, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = \
                    _to_sph(mol, i, j, v[c].reshape(3, si.ncart, sj.ncart))
    return out


def hcore_generator(mol):
    """``hcore_deriv(ia)`` -> (3, nao, nao) as PySCF ``grad.rhf.hcore_generator``: the basis-function
    derivatives -<nabla mu|T + V_ne|nu> on the rows of atom ia's AOs plus the derivative of atom
    ia's own attraction -Z <nabla mu|1/|r - R_ia||nu>, symmetrised."""
    vat = iprinv_atoms(mol)
    h1 = -(ipkin(mol) + vat.sum(axis=0))
    on = mol.ao_atom()

    def hcore_deriv(ia):
        v = vat[ia].copy()
        rows = on == ia
        v[:, rows] += h1[:, rows]
        return v + v.transpose(0, 2, 1)
    return hcore_deriv


def grad_nuc(mol, atmlst=None):
    """Derivative of the nuclear repulsion, (natm, 3)."""
    Z, R = mol._charges, mol.atom_coords()
    g = np.zeros((mol.natm, 3))
    for i in range(mol.natm):
        for j in range(mol.natm):
            if i != j:
                d = R[i] - R[j]
                g[i] -= Z[i] * Z[j] * d / np.linalg.norm(d) ** 3
    return g if atmlst is None else g[list(atmlst)]


# ------------------------------------------------------------------ the two-electron contraction
def jk_terms(cj, ck, d, dprime):
    """The kernel term of ``sum_{p on A} (cj vj[D] + ck vk[D])[x,p,q] (D'[p,q] + D'[q,p])`` with
    PySCF's vj / vk above: (wj, wk, P, Q).  A term carrying both needs a symmetric D (J reads
    D^T, K reads D)."""
    d = np.asarray(d, dtype=np.float64)
    dp = np.asarray(dprime, dtype=np.float64)
    if cj != 0 and ck != 0 and np.abs(d - d.T).max() > 1e-12 * max(1.0, np.abs(d).max()):
        raise ValueError("a combined J / K term needs a symmetric density")
    return (-float(cj), -float(ck), dp + dp.T, d.T if ck == 0 else d)


def cart_transform(mol):
    """(nao, ncart_ao) block-diagonal C with chi_mu = sum_a C[mu, a] g_a over the Cartesian
    components of the shells (AO norms included), and the first Cartesian component per shell."""
    cloc = np.cumsum([0] + [s.ncart for s in mol.shells])
    C = np.zeros((mol.nao, cloc[-1]))
    for k, s in enumerate(mol.shells):
        p0, p1 = mol.ao_loc[k], mol.ao_loc[k + 1]
        C[p0:p1, cloc[k]:cloc[k + 1]] = _sph_transform(s.l) * mol._norm[p0:p1, None]
    return C, cloc


class GradTables:
    """Side arrays of ``xt_grad_jk`` next to the existing tables: for every ordered bra entry of
    ``DerivPairTable`` the Cartesian AO offsets of a and b, ncart(b) and the atom of a; for every
    ket pair c >= d of ``PairTable`` the offsets of c and d, ncart(d) and whether c != d; and
    the contiguous ranges of both tables per dispatch bucket (both are sorted by order)."""

    def __init__(self, mol):
        from .dints import deriv_pair_table, pair_table
        self.mol = mol
        self.bra = deriv_pair_table(mol, False, False)
        self.ket = pair_table(mol)
        self.cmat, cloc = cart_transform(mol)
        self.ncart = int(cloc[-1])
        sh = mol.shells
        self.bra_ao = np.array([[cloc[i], cloc[j], sh[j].ncart, sh[i].atom] for i, j in self.bra.pairs],
                               dtype=np.int32)
        self.ket_ao = np.array([[cloc[i], cloc[j], sh[j].ncart, int(i != j)] for i, j in self.ket.pairs],
                               dtype=np.int32)
        self.ket_info = self.ket.ket_info_pairs(np.arange(self.ket.npair), self.ket.c0.astype(np.int32))
        self.bra_ranges = _ranges(self.bra.info[:, 0], BRA_BOUNDS)
        self.ket_ranges = _ranges(self.ket_info[:, 0], KET_BOUNDS)
        self._dev = {}

    def dev(self, device):
        if device not in self._dev:
            import torch
            dv = torch.device(f"cuda:{device}")
            self._dev[device] = dict(bra_ao=torch.as_tensor(self.bra_ao, device=dv),
                                     ket_ao=torch.as_tensor(self.ket_ao, device=dv),
                                     ket_info=torch.as_tensor(self.ket_info, device=dv))
        return self._dev[device]


def _ranges(orders, bounds):
    """[(first, end, largest order)] of the entries of each bucket; ``orders`` ascending."""
    orders = np.asarray(orders)
    if np.any(np.diff(orders) < 0):
        raise ValueError("table not sorted by order")
    out, lo = [], 0
    for b in bounds:
        hi = int(np.searchsorted(orders, b, side="right"))
        if hi > lo:
            out.append((lo, hi, int(orders[hi - 1])))
        lo = hi
    if lo != orders.size:
        raise ValueError(f"shells above f: order {int(orders.max())}")
    return out


def grad_tables(mol) -> GradTables:
    tab = getattr(mol, "_grad_tables", None)
    if tab is None:
        tab = GradTables(mol)
        mol._grad_tables = tab
    return tab


def default_strip(nbra, nket):
    """Ket entries per thread: the shortest strip that still leaves 2^16 threads."""
    return int(max(1, min(64, nbra * nket // 65536)))


def work_size(nbra, nket, strip):
    """Doubles of workspace one ``xt_grad_jk`` launch needs (``grad_jk_work`` of csrc/xt_grad.hip):
    the partial sums of every strip and the per-entry sums."""
    return 3 * nbra * ((nket + strip - 1) // strip + 1)


def grad_jk_device(mol, terms, device: int = 0, strip=None, stats=None):
    """(natm, 3): sum over ``terms`` = [(wj, wk, P, Q)] (P, Q (nao, nao) over the spherical AOs,
    arbitrary) of the derivative-ERI contraction in the module docstring, through ``xt_grad_jk``.
    The bra tables (``ints.deriv_tables``) hold the derivative with respect to the centre of a, so
    the kernel's sum is negated here.  The densities are transformed to the Cartesian components once; the launches of the
    (bra bucket, ket bucket) ranges add into one (natm, 3) array in a fixed order.
    ``stats``: a dict that receives quartets and wall ms per bucket pair."""
    import torch
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"xt_grad_jk takes 1..{MAX_TERMS} terms, got {len(terms)}")
    L = _capi.lib()
    tab = grad_tables(mol)
    dv = torch.device(f"cuda:{device}")
    C = tab.cmat
    wj = np.array([t[0] for t in terms], dtype=np.float64)
    wk = np.array([t[1] for t in terms], dtype=np.float64)
    P = np.stack([C.T @ np.asarray(t[2], dtype=np.float64) @ C for t in terms])
    Q = np.stack([C.T @ np.asarray(t[3], dtype=np.float64) @ C for t in terms])
    with torch.cuda.device(dv):
        b, k, g = tab.bra.dev(device), tab.ket.dev(device), tab.dev(device)
        tP, tQ = torch.as_tensor(P, device=dv), torch.as_tensor(Q, device=dv)
        out = torch.zeros((mol.natm, 3), dtype=torch.float64, device=dv)
        st = ctypes.c_void_p(torch.cuda.current_stream(dv).cuda_stream)
        for b0, b1, lb in tab.bra_ranges:
            for k0, k1, lk in tab.ket_ranges:
                nb, nk = b1 - b0, k1 - k0
                sl = default_strip(nb, nk) if strip is None else int(strip)
                nwork = work_size(nb, nk, sl)
                work = torch.empty(nwork, dtype=torch.float64, device=dv)
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    t0 = time.perf_counter()
                _capi.check(L.xt_grad_jk(nb, b["info"][b0:].data_ptr(), b["prim"].data_ptr(), b["eb"].data_ptr(),
                                         g["bra_ao"][b0:].data_ptr(), nk, g["ket_info"][k0:].data_ptr(),
                                         k["pprim"].data_ptr(), k["eab"].data_ptr(), g["ket_ao"][k0:].data_ptr(),
                                         lb, lk, len(terms), wj.ctypes.data, wk.ctypes.data, tP.data_ptr(),
                                         tQ.data_ptr(), tab.ncart, sl, mol.natm, work.data_ptr(), nwork,
                                         out.data_ptr(), st), "xt_grad_jk")
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    stats.setdefault("buckets", []).append(dict(
                        bra_order=lb, ket_order=lk, quartets=nb * nk, strip=sl,
                        ms=(time.perf_counter() - t0) * 1e3))
        return -out.cpu().numpy()


# ------------------------------------------------------------------ Z-vector
def gmres(aop, b, precond, tol, max_cycle):
    """Solve aop(x) = b by left-preconditioned full GMRES from x = 0; returns (x, residual norm
    |aop(x) - b|_2, cycles).  Raises when the residual stays above ``tol`` after ``max_cycle``
    applications of ``aop``."""
    r0 = precond(b)
    beta = np.linalg.norm(r0)
    if beta == 0.0:
        return np.zeros_like(b), 0.0, 0
    V = [r0 / beta]
    AV = []                      # un-preconditioned products, for the true residual
    H = np.zeros((max_cycle + 1, max_cycle))
    x = np.zeros_like(b)
    res = np.linalg.norm(b)
    for k in range(max_cycle):
        av = aop(V[k])
        AV.append(av)
        w = precond(av)
        for i in range(k + 1):
            H[i, k] = V[i] @ w
            w = w - H[i, k] * V[i]
        for i in range(k + 1):   # second Gram-Schmidt pass
            c = V[i] @ w
            H[i, k] += c
            w = w - c * V[i]
        H[k + 1, k] = np.linalg.norm(w)
        e1 = np.zeros(k + 2)
        e1[0] = beta
        y = np.linalg.lstsq(H[:k + 2, :k + 1], e1, rcond=None)[0]
        x = sum(yi * vi for yi, vi in zip(y, V))
        res = np.linalg.norm(sum(yi * avi for yi, avi in zip(y, AV)) - b)
        if res <= tol:
            return x, res, k + 1
        if H[k + 1, k] <= 1e-300:
            raise RuntimeError(f"Z-vector equations: the Krylov space broke down after {k + 1} cycles at "
                               f"residual {res:.3e} > {tol:.1e}")
        V.append(w / H[k + 1, k])
    raise RuntimeError(f"Z-vector equations not converged in {max_cycle} cycles: residual {res:.3e} > {tol:.1e}")


def uhf_orbitals(mf):
    """(orbo_a, orbv_a, orbo_b, orbv_b, fock_mo_a, fock_mo_b) of a converged UHF."""
    out = []
    for s in range(2):
        c, occ = mf.mo_coeff[s], mf.mo_occ[s]
        out += [c[:, occ > 0], c[:, occ == 0]]
    f = mf.get_hcore()[None] + np.asarray(mf._veff)
    return (*out, mf.mo_coeff[0].T @ f[0] @ mf.mo_coeff[0], mf.mo_coeff[1].T @ f[1] @ mf.mo_coeff[1])


def hf_response(mf):
    """vresp(dm (2, nao, nao) symmetric) = J[dm_a + dm_b] - K[dm_s] (``mf.gen_response(hermi=1)``
    of a UHF mean field); J / K from the mean field's engine (the device's after to_device())."""
    def vresp(dm):
        vj, vk = mf.get_jk(dm=np.asarray(dm), hermi=1)
        return (vj[0] + vj[1])[None] - vk
    return vresp


def solve_zvector(mf, wvoa, wvob, tol=1e-10, max_cycle=500):
    """z (vo blocks of both spins) with fvind(z) = -(wvoa, wvob) (usfcis.py:126-150): (A + B) of
    the UHF reference, preconditioned by the orbital-energy differences.  Returns
    (z1a, z1b, residual, cycles)."""
    orboa, orbva, orbob, orbvb, fa, fb = uhf_orbitals(mf)
    nocca, nvira, noccb, nvirb = orboa.shape[1], orbva.shape[1], orbob.shape[1], orbvb.shape[1]
    vresp = hf_response(mf)
    na = nvira * nocca

    def fvind(x):
        xa = x[:na].reshape(nvira, nocca)
        xb = x[na:].reshape(nvirb, noccb)
        dma = orbva @ xa @ orboa.T
        dmb = orbvb @ xb @ orbob.T
        v1 = vresp(np.asarray([(dma + dma.T) / 2, (dmb + dmb.T) / 2])) * 2
        v1a = orbva.T @ v1[0] @ orboa + fa[nocca:, nocca:].T @ xa - xa @ fa[:nocca, :nocca].T
        v1b = orbvb.T @ v1[1] @ orbob + fb[noccb:, noccb:].T @ xb - xb @ fb[:noccb, :noccb].T
        return np.hstack((v1a.ravel(), v1b.ravel()))
    ea, eb = mf.mo_energy
    diag = np.hstack(((ea[nocca:, None] - ea[None, :nocca]).ravel(), (eb[noccb:, None] - eb[None, :noccb]).ravel()))
    diag = np.where(np.abs(diag) < 1e-8, 1e-8, diag)
    w = -np.hstack((np.asarray(wvoa).ravel(), np.asarray(wvob).ravel()))
    z, res, ncyc = gmres(fvind, w, lambda v: v / diag, tol, max_cycle)
    return z[:na].reshape(nvira, nocca), z[na:].reshape(nvirb, noccb), res, ncyc


# ------------------------------------------------------------------ UHF ground state
def check_gradient_mf(mf):
    """The mean fields the gradients here cover: unrestricted, Hartree-Fock, exact integrals."""
    if getattr(mf, "restricted_open", False):
        raise NotImplementedError("nuclear gradients need a UHF reference: an ROHF / ROKS determinant is "
                                  "not variational in the rotations the formula assumes")
    xc = str(getattr(mf, "xc", "HF")).upper()
    if xc != "HF":
        raise NotImplementedError(f"nuclear gradients for xc = {mf.xc!r}: the XC derivative terms are not built "
                                  "(Hartree-Fock only)")
    if getattr(mf, "with_df", None) is not None:
        raise NotImplementedError("nuclear gradients for density-fitted mean fields")
    if getattr(mf, "with_x2c", None) is not None:
        raise NotImplementedError("nuclear gradients with the X2C core Hamiltonian")
    # J / K from the integral-direct Cholesky factor are exact to chol_tol only, while xt_grad_jk
    # differentiates the exact integrals: a loose factor would give a non-variational gradient
    uses_chol = getattr(mf, "cderi_exact", None) is not None or getattr(mf, "eri_mode", "") == "cholesky"
    if uses_chol and float(getattr(mf, "chol_tol", 0.0)) > MAX_CHOL_TOL:
        raise ValueError(f"nuclear gradients need J / K of the exact integrals: Cholesky tolerance "
                         f"{mf.chol_tol:g} is above {MAX_CHOL_TOL:g}")


def ground_terms(d0a, d0b):
    """The three kernel terms of the UHF two-electron gradient: J[D_a + D_b] with D_a + D_b,
    -K[D_a] with D_a, -K[D_b] with D_b."""
    d0t = d0a + d0b
    return [jk_terms(1, 0, d0t, d0t), jk_terms(0, -1, d0a, d0a), jk_terms(0, -1, d0b, d0b)]


def contract_1e(mol, hcore_deriv, s1, dm_h, w):
    """sum_pq h1(A)[x,p,q] dm_h[p,q] - sum_{p on A, q} s1[x,p,q] (w[p,q] + w[q,p]): (natm, 3)."""
    on = mol.ao_atom()
    de = np.zeros((mol.natm, 3))
    ws = w + w.T
    for ia in range(mol.natm):
        rows = on == ia
        de[ia] = np.einsum('xpq,pq->x', hcore_deriv(ia), dm_h) - np.einsum('xpq,pq->x', s1[:, rows], ws[rows])
    return de


class Gradients:
    """``UHF.nuc_grad_method()``: ``kernel()`` -> (natm, 3) dE/dR in Ha / Bohr.  The two-electron
    part is one ``xt_grad_jk`` call on the mean field's device (``mf.to_device()``)."""

    def __init__(self, mf):
        check_gradient_mf(mf)
        self.base = mf
        self.mol = mf.mol
        self.atmlst = None
        self.de = None
        self.timings = {}

    def get_ovlp(self, mol=None):
        return get_ovlp(mol or self.mol)

    def hcore_generator(self, mol=None):
        return hcore_generator(mol or self.mol)

    def grad_nuc(self, mol=None, atmlst=None):
        return grad_nuc(mol or self.mol, atmlst)

    def _device(self):
        dev = getattr(self.base, "_device", None)
        if dev is None:
            raise RuntimeError("the two-electron gradient runs on the GPU (xt_grad_jk): call mf.to_device() "
                               "before kernel()")
        return dev

    def grad_elec(self, atmlst=None):
        mf, mol = self.base, self.mol
        if mf.mo_coeff is None:
            raise RuntimeError("run the SCF first")
        dev = self._device()
        orboa, _, orbob, _, fa, fb = uhf_orbitals(mf)
        nocca, noccb = orboa.shape[1], orbob.shape[1]
        d0a, d0b = orboa @ orboa.T, orbob @ orbob.T
        w = orboa @ fa[:nocca, :nocca] @ orboa.T + orbob @ fb[:noccb, :noccb] @ orbob.T
        t0 = time.perf_counter()
        de = contract_1e(mol, hcore_generator(mol), get_ovlp(mol), d0a + d0b, w)
        self.timings["one_electron_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        st = {}
        de += grad_jk_device(mol, ground_terms(d0a, d0b), dev, stats=st)
        self.timings["grad_jk_s"] = time.perf_counter() - t0
        self.timings["buckets"] = st.get("buckets", [])
        return de if atmlst is None else de[list(atmlst)]

    def kernel(self, atmlst=None):
        if atmlst is None:
            atmlst = self.atmlst
        else:
            self.atmlst = atmlst
        self.de = self.grad_elec(atmlst) + self.grad_nuc(atmlst=atmlst)
        return self.de
