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
* ``grad_jk_lists`` -- the same contraction with separate Coulomb and exchange pair lists
  (``xt_grad_jk2``), for the two-particle densities of more than eight pairs (``xtddft_amd/grad_utda.py``);
* ``grad_jk_rsh`` -- the two calls of a range-separated hybrid: ``xt_grad_jk2`` with hyb on the exchange
  list and ``xt_grad_jk2_lr`` (erf(omega r12) / r12) with alpha - hyb on the same pairs;
* ``grad_2e`` -- the one place that chooses among the three above and fills the timing keys, for the ground
  states here and the excited-state drivers; ``exchange_jk`` -- J and hyb K + (alpha - hyb) K_LR of
  non-symmetric densities, the ``get_jk`` of both excited-state ``grad_elec``;
* ``solve_zvector`` -- the UCPHF Z-vector equations (usfcis.py:127-150) by a host-driven
  preconditioned GMRES whose response J / K come from ``DeviceEngine.get_jk``;
* ``Gradients`` -- ``UHF.nuc_grad_method()``: the T = Z = X = 0 subset of the excited-state
  formula with W the energy-weighted density;
* ``grad_xc_device`` -- the nuclear derivative of the XC potential matrix contracted with the
  ground-state density (PySCF ``grad.uks.get_vxc``; the ``vxc1[:, 1:]`` of the reference's
  ``grad_hb/tduks_sfu.py:168-177``) on a grid held fixed in space, through the engine's GEMMs and
  the library kernel ``xt_grad_xc`` (``csrc/xt_grad_xc.hip``),

      g[A, x] = -2 sum_s sum_g sum_{mu on A} d_x phi_mu e_s[g, mu] + (sum_k h_s[k, g] d_x d_k phi_mu) c_s[g, mu]

  with h_s = w vxc_s in the "eff" layout (d eps / d rho_s, d eps / d(d_k rho_s); nothing halved),
  b_s = h_s[0] phi + sum_k h_s[k] d_k phi, e_s = b_s D_s and c_s = phi D_s;
* ``KSGradients`` -- ``UKS.nuc_grad_method()`` after ``to_device()``: LDA / GGA functionals, pure
  and global hybrid, without grid-weight derivatives (``grid_response = False``);
* ``grad_xc_pairs`` -- the same bracket for any list of (weights h, densities D): G_xc[h; D] is
  bilinear, and the excited-state gradients of ``xtddft_amd/grad.py`` need it at
  (w vxc[rho0], D0 + T + Z^S) and at (wv[T + Z^S], D0);
* ``ks_response`` -- the response of a UKS mean field to a symmetric density pair,
  J - hyb K + V^resp (``DeviceEngine.fxc_response``, kernel ``xt_xc_resp``), which ``solve_zvector``
  takes through its ``vresp`` argument.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np

from .. import _capi
from . import xc as _xc
from .gto import _sph_transform
from .ints import DerivPair, hermite_r, kinetic_deriv1

MAX_TERMS = 8
MAX_CHOL_TOL = 1e-10     # loosest ERI Cholesky tolerance a gradient accepts (check_gradient_mf)
XC_TILE = 64             # grid points per block of xt_grad_xc in GGA mode (csrc/xt_grad_xc.hip)
XC_CHUNK_BYTES = 1 << 28  # e and c of one grid chunk of grad_xc_device stay below this
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


def _launch_buckets(mol, device, strip, stats, name, make_call):
    """The launches both entries of the kernel share: for every (bra bucket, ket bucket) range of the
    tables one call with its own workspace, all adding into one (natm, 3) array in a fixed order, whose
    negative is returned (the bra tables hold the derivative with respect to the centre of a).
    ``make_call(dv, tab)`` puts the densities on the device and returns ``call(head, tail)``: the C entry
    with the table arguments ``head``, its own density arguments, and ``tail`` (nao, strip, natm, work,
    nwork, out, stream).  ``stats``: a dict that receives quartets and wall ms per bucket pair."""
    import torch
    tab = grad_tables(mol)
    dv = torch.device(f"cuda:{device}")
    with torch.cuda.device(dv):
        b, k, g = tab.bra.dev(device), tab.ket.dev(device), tab.dev(device)
        call = make_call(dv, tab)
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
                head = (nb, b["info"][b0:].data_ptr(), b["prim"].data_ptr(), b["eb"].data_ptr(),
                        g["bra_ao"][b0:].data_ptr(), nk, g["ket_info"][k0:].data_ptr(), k["pprim"].data_ptr(),
                        k["eab"].data_ptr(), g["ket_ao"][k0:].data_ptr(), lb, lk)
                tail = (tab.ncart, sl, mol.natm, work.data_ptr(), nwork, out.data_ptr(), st)
                _capi.check(call(head, tail), name)
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    stats.setdefault("buckets", []).append(dict(
                        bra_order=lb, ket_order=lk, quartets=nb * nk, strip=sl,
                        ms=(time.perf_counter() - t0) * 1e3))
        return -out.cpu().numpy()


def _cart_stack(tab, dv, terms, i):
    """The matrices ``t[i]`` of ``terms`` over the Cartesian components, stacked on the device; None
    for an empty list."""
    import torch
    if not terms:
        return None
    C = tab.cmat
    return torch.as_tensor(np.stack([C.T @ np.asarray(t[i], dtype=np.float64) @ C for t in terms]), device=dv)


def grad_jk_device(mol, terms, device: int = 0, strip=None, stats=None):
    """(natm, 3): sum over ``terms`` = [(wj, wk, P, Q)] (P, Q (nao, nao) over the spherical AOs,
    arbitrary) of the derivative-ERI contraction in the module docstring, through ``xt_grad_jk``.
    The bra tables (``ints.deriv_tables``) hold the derivative with respect to the centre of a, so
    the kernel's sum is negated here.  The densities are transformed to the Cartesian components once; the launches of the
    (bra bucket, ket bucket) ranges add into one (natm, 3) array in a fixed order.
    ``stats``: a dict that receives quartets and wall ms per bucket pair."""
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"xt_grad_jk takes 1..{MAX_TERMS} terms, got {len(terms)}")
    L = _capi.lib()
    wj = np.array([t[0] for t in terms], dtype=np.float64)
    wk = np.array([t[1] for t in terms], dtype=np.float64)

    def make_call(dv, tab):
        tP, tQ = _cart_stack(tab, dv, terms, 2), _cart_stack(tab, dv, terms, 3)
        return lambda head, tail: L.xt_grad_jk(*head, len(terms), wj.ctypes.data, wk.ctypes.data, tP.data_ptr(),
                                               tQ.data_ptr(), *tail)
    return _launch_buckets(mol, device, strip, stats, "xt_grad_jk", make_call)


def grad_jk_lists(mol, jterms, kterms, device: int = 0, strip=None, stats=None, omega: float = 0.0):
    """(natm, 3): ``grad_jk_device`` with a Coulomb list ``jterms`` = [(wj, P, Q)] and an exchange list
    ``kterms`` = [(wk, P, Q)] of their own, through ``xt_grad_jk2``,

        g[A, m] = sum_{a on A} sum_{bcd} (d_m a  b|c d) (sum_t wj_t P_t[a,b] Q_t[c,d] + sum_t wk_t P_t[a,c] Q_t[b,d]);

    up to ``MAX_TERMS`` pairs in each list, at least one pair in all, one pass over the derivative
    integrals.  An empty list is handed over as null pointers (a pure functional passes no exchange).
    Sign, transformation to Cartesian components, launch order and ``stats`` as ``grad_jk_device``.
    ``omega`` > 0: the derivative integrals over erf(omega r12) / r12, through ``xt_grad_jk2_lr`` (the
    long-range exchange of a range-separated hybrid, ``grad_jk_rsh``); the default 0 is 1/r12."""
    jterms, kterms = list(jterms), list(kterms)
    nj, nk = len(jterms), len(kterms)
    omega = float(omega)
    name = "xt_grad_jk2_lr" if omega > 0 else "xt_grad_jk2"
    if nj > MAX_TERMS or nk > MAX_TERMS or nj + nk < 1:
        raise ValueError(f"{name} takes 0..{MAX_TERMS} Coulomb and 0..{MAX_TERMS} exchange pairs, at least one "
                         f"in all, got {nj} and {nk}")
    if not (np.isfinite(omega) and omega >= 0.0):
        raise ValueError(f"omega must be finite and >= 0, got {omega!r}")
    L = _capi.lib()
    wj = np.array([t[0] for t in jterms], dtype=np.float64)
    wk = np.array([t[0] for t in kterms], dtype=np.float64)

    def ptr(x):
        return None if x is None else x.data_ptr()

    def make_call(dv, tab):
        pj, qj = _cart_stack(tab, dv, jterms, 1), _cart_stack(tab, dv, jterms, 2)
        pk, qk = _cart_stack(tab, dv, kterms, 1), _cart_stack(tab, dv, kterms, 2)

        def lists():             # the closure keeps the device matrices alive for as long as the call exists
            return (nj, wj.ctypes.data if nj else None, ptr(pj), ptr(qj),
                    nk, wk.ctypes.data if nk else None, ptr(pk), ptr(qk))
        if omega > 0:
            return lambda head, tail: L.xt_grad_jk2_lr(*head, *lists(), *tail, omega)
        return lambda head, tail: L.xt_grad_jk2(*head, *lists(), *tail)
    return _launch_buckets(mol, device, strip, stats, name, make_call)


def pair_lists(terms):
    """``grad_jk_device`` terms [(wj, wk, P, Q)] as the two lists of ``grad_jk_lists``: (Coulomb list
    [(wj, P, Q)] of the terms with wj != 0, exchange list [(wk, P, Q)] of those with wk != 0)."""
    return ([(wj, p, q) for wj, _, p, q in terms if wj != 0], [(wk, p, q) for _, wk, p, q in terms if wk != 0])


def grad_jk_rsh(mol, jterms, kterms, omega, hyb, alpha, device: int = 0, strip=None, stats=None):
    """(natm, 3): the two-electron derivative term of a range-separated hybrid, whose exchange is
    hyb K + (alpha - hyb) K_LR (``qc/scf.py`` ``get_veff``).  ``jterms`` = [(wj, P, Q)] and ``kterms`` =
    [(wk, P, Q)] are the lists of ``grad_jk_lists`` with the exchange weights of FULL exchange (hyb = 1).
    Two passes over the derivative integrals:

    1. ``xt_grad_jk2`` (1/r12) with the Coulomb list and the exchange list weighted by ``hyb``;
    2. ``xt_grad_jk2_lr`` (erf(omega r12) / r12) with no Coulomb pair and the same exchange pairs weighted
       by ``alpha - hyb``.

    Call 2 runs alone where hyb = 0 and the Coulomb list is empty; call 1 alone where alpha = hyb.
    ``stats``: the buckets of call 1 under ``buckets``, those of call 2 under ``buckets_lr``, and the wall
    seconds of either under ``full_s`` / ``lr_s``."""
    jterms, kterms = list(jterms), list(kterms)
    if not omega > 0:
        raise ValueError("grad_jk_rsh is for a range-separated functional (omega > 0); a global hybrid is "
                         "one grad_jk_lists call")
    de = np.zeros((mol.natm, 3))
    k_full = [(hyb * w, p, q) for w, p, q in kterms] if hyb != 0 else []
    k_lr = [((alpha - hyb) * w, p, q) for w, p, q in kterms] if alpha != hyb else []
    if jterms or k_full:
        st = None if stats is None else {}
        t0 = time.perf_counter()
        de += grad_jk_lists(mol, jterms, k_full, device, strip, st)
        if stats is not None:
            stats["full_s"] = time.perf_counter() - t0
            stats.setdefault("buckets", []).extend(st.get("buckets", []))
    if k_lr:
        st = None if stats is None else {}
        t0 = time.perf_counter()
        de += grad_jk_lists(mol, [], k_lr, device, strip, st, omega=omega)
        if stats is not None:
            stats["lr_s"] = time.perf_counter() - t0
            stats.setdefault("buckets_lr", []).extend(st.get("buckets", []))
    return de


def grad_2e(mol, device, timings, hyb=1.0, rsh=None, *, terms=None, lists=None):
    """(natm, 3): the two-electron derivative term of every gradient driver, given either as ``terms`` =
    [(wj, wk, P, Q)] or as ``lists`` = (Coulomb list, exchange list).  Without range separation the terms go
    through ``grad_jk_device`` (``xt_grad_jk``) and the lists through ``grad_jk_lists`` (``xt_grad_jk2``), with
    ``hyb`` already in their exchange weights.  ``rsh`` = (omega, alpha): the exchange weights are those of full
    exchange and either form goes as two lists through ``grad_jk_rsh``, which weights them with ``hyb`` and
    alpha - hyb.  ``timings`` receives ``grad_jk_s`` and ``buckets`` and, with ``rsh``, ``grad_jk_full_s``,
    ``grad_jk_lr_s`` and ``buckets_lr``."""
    t0 = time.perf_counter()
    st = {}
    if rsh is not None:
        jl, kl = pair_lists(terms) if lists is None else lists
        de = grad_jk_rsh(mol, jl, kl, float(rsh[0]), hyb, float(rsh[1]), device, stats=st)
        timings["grad_jk_full_s"], timings["grad_jk_lr_s"] = st.get("full_s"), st.get("lr_s")
        timings["buckets_lr"] = st.get("buckets_lr", [])
    elif lists is None:
        de = grad_jk_device(mol, terms, device, stats=st)
    else:
        de = grad_jk_lists(mol, *lists, device, stats=st)
    timings["grad_jk_s"] = time.perf_counter() - t0
    timings["buckets"] = st.get("buckets", [])
    return de


def exchange_jk(scf, hyb, rsh=None):
    """``get_jk(dms)`` -> (J, the exchange of the functional) of a stack of densities that need not be
    symmetric: hyb K and, with ``rsh`` = (omega, alpha) of a range-separated hybrid, hyb K + (alpha - hyb) K_LR
    (``scf.get_k_lr``).  hyb = 0 forms no full-range exchange (``with_k=False``).  J / K do not depend on
    which spin a density belongs to."""
    k_lr = 0.0 if rsh is None else float(rsh[1]) - hyb

    def get_jk(dms):
        dms = np.asarray(dms)
        if k_lr != 0:            # get_k_lr takes non-symmetric densities
            vk_lr = k_lr * np.asarray(scf.get_k_lr(dms))
            if hyb == 0:
                return scf.get_jk(dm=dms, hermi=0, with_k=False)[0], vk_lr
            vj, vk = scf.get_jk(dm=dms, hermi=0)
            return vj, hyb * vk + vk_lr
        if hyb == 0:             # a pure functional forms no exchange
            return scf.get_jk(dm=dms, hermi=0, with_k=False)[0], np.zeros_like(dms)
        vj, vk = scf.get_jk(dm=dms, hermi=0)
        return vj, (vk if hyb == 1 else hyb * vk)
    return get_jk


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


def ks_response(mf):
    """vresp(dm (2, nao, nao) symmetric) = J[dm_a + dm_b] - hyb K[dm_s] + V^resp_s[dm]
    (``mf.gen_response(hermi=1)`` of a UKS mean field, LDA / GGA, global hybrid or pure): J / K from
    ``mf.get_jk`` and the XC response from ``DeviceEngine.fxc_response`` with fxc at the SCF
    density.  A pure functional forms no exchange; a range-separated one (``mf.omega`` != 0) adds
    -(alpha - hyb) K_LR[dm_s] (``mf.get_k_lr``)."""
    eng = getattr(mf, "device_engine", None)
    if eng is None:
        raise RuntimeError("ks_response needs a built Kohn-Sham mean field on a device (mf.to_device())")
    hyb = float(mf.hyb)
    k_lr = float(mf.alpha) - hyb if float(getattr(mf, "omega", 0.0)) != 0 else 0.0
    eng.fxc_ground(np.asarray(mf.make_rdm1()))

    def vresp(dm):
        dm = np.asarray(dm)
        vxc = eng.fxc_response(dm, want=("v",))["v"]
        if k_lr != 0:
            vxc = vxc - k_lr * np.asarray(mf.get_k_lr(dm))
        if hyb != 0:
            vj, vk = mf.get_jk(dm=dm, hermi=1)
            return (vj[0] + vj[1])[None] - hyb * vk + vxc
        vj = mf.get_jk(dm=dm, hermi=1, with_k=False)[0]
        return (vj[0] + vj[1])[None] + vxc
    return vresp


def solve_zvector(mf, wvoa, wvob, tol=1e-10, max_cycle=500, vresp=None):
    """z (vo blocks of both spins) with fvind(z) = -(wvoa, wvob) (usfcis.py:126-150): (A + B) of
    the reference, preconditioned by the orbital-energy differences.  ``vresp``: the response of
    the mean field to a symmetric density pair, default ``hf_response(mf)`` (a UKS reference passes
    ``ks_response``).  Returns (z1a, z1b, residual, cycles)."""
    orboa, orbva, orbob, orbvb, fa, fb = uhf_orbitals(mf)
    nocca, nvira, noccb, nvirb = orboa.shape[1], orbva.shape[1], orbob.shape[1], orbvb.shape[1]
    if vresp is None:
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
    _check_exact_integrals(mf)


def _check_exact_integrals(mf):
    """The last refusals of both ``check_gradient_mf`` and ``check_ks_gradient_mf``: density fitting, X2C and
    a loose Cholesky factor."""
    if getattr(mf, "with_df", None) is not None:
        raise NotImplementedError("nuclear gradients for density-fitted mean fields")
    if getattr(mf, "with_x2c", None) is not None:
        raise NotImplementedError("nuclear gradients with the X2C core Hamiltonian")
    # J / K from the integral-direct Cholesky factor are exact to chol_tol only, while xt_grad_jk
    # differentiates the exact integrals: a loose factor would give a non-variational gradient; the
    # long-range factor of a range-separated functional is built at the same chol_tol
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
        self._check_mf(mf)
        self.base = mf
        self.mol = mf.mol
        self.atmlst = None
        self.de = None
        self.timings = {}

    def _check_mf(self, mf):
        check_gradient_mf(mf)

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

    def _one_electron(self):
        """(the device, D_a, D_b, the one-electron and overlap part (natm, 3)) of a converged mean field: the
        energy-weighted density is that of ``mf._veff``, which on a UKS holds V_xc + J - hyb K."""
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
        return dev, d0a, d0b, de

    def grad_elec(self, atmlst=None):
        dev, d0a, d0b, de = self._one_electron()
        de += grad_2e(self.mol, dev, self.timings, terms=ground_terms(d0a, d0b))
        return de if atmlst is None else de[list(atmlst)]

    def kernel(self, atmlst=None):
        if atmlst is None:
            atmlst = self.atmlst
        else:
            self.atmlst = atmlst
        self.de = self.grad_elec(atmlst) + self.grad_nuc(atmlst=atmlst)
        return self.de


# ------------------------------------------------------------------ UKS ground state
def xc_work_size(ngrid, nshell):
    """Doubles of workspace one ``xt_grad_xc`` call needs (``grad_xc_work`` of csrc/xt_grad_xc.hip)."""
    return 3 * nshell * ((ngrid + XC_TILE - 1) // XC_TILE + 1)


def default_xc_chunk(nao, ngrid):
    """Grid points per ``xt_grad_xc`` call: the largest multiple of 256 at which e and c of both
    spins (4 nao doubles per point) stay below ``XC_CHUNK_BYTES``, at least 256, at most the grid."""
    return int(min(max(ngrid, 1), max(256, XC_CHUNK_BYTES // (32 * max(nao, 1)) // 256 * 256)))


def grad_xc_device(mf, d0a, d0b, chunk=None, stats=None):
    """(natm, 3): the XC part of the UKS gradient at the spin densities d0a, d0b on the mean
    field's grid, points and weights held fixed (module docstring).  rho and vxc come from the
    device engine; per chunk of ``chunk`` grid points (``default_xc_chunk``) the products
    e_s = D_s b_s^T and c_s = D_s phi^T run on the engine's FP64 MFMA GEMM in the AO-major layout
    the kernel reads, then one ``xt_grad_xc`` call adds the chunk's force.  ``stats``: a dict that
    receives the seconds of the GEMMs and of the kernel and the bytes of h, e and c it read."""
    def items(eng, t):
        dms = t(np.asarray([d0a, d0b], dtype=np.float64))
        rho = eng.torch.stack([eng._rho(dms[0]), eng._rho(dms[1])])
        vxc = _xc.eval_xc_eff_torch(mf.xc, rho, deriv=1)[1]
        return [(vxc * eng.w, dms)]                                              # h: (2, ncomp, G)
    return _grad_xc_run(mf, items, chunk, stats)


def grad_xc_pairs(mf, pairs, chunk=None, stats=None):
    """(natm, 3): sum over ``pairs`` = [(h, (Da, Db))] of the bracket of ``grad_xc_device`` with the
    weights h (2, ncomp, G) on the device ("eff" layout, nothing halved) and the densities
    (Da + Da^T) / 2, (Db + Db^T) / 2 -- G_xc[h; D], bilinear in both.  ``grad_xc_device(mf, d0a, d0b)``
    is the single pair (w vxc[rho0], D0); the excited-state gradients add (wv[T + Z^S], D0).  The
    chunk loop runs once per pair and every pair adds into the same (natm, 3) array."""
    pairs = list(pairs)
    if not pairs:
        raise ValueError("grad_xc_pairs needs at least one (h, (Da, Db)) pair")

    def items(eng, t):
        ng, ncomp = int(eng.w.shape[0]), (4 if mf.xctype == "GGA" else 1)
        out = []
        for h, (da, db) in pairs:
            da, db = np.asarray(da, dtype=np.float64), np.asarray(db, dtype=np.float64)
            h = eng.torch.as_tensor(h, dtype=eng.torch.float64, device=eng.dev)
            if h.dim() != 3 or h.shape[0] != 2 or h.shape[1] < ncomp or h.shape[2] != ng:
                raise ValueError(f"grad_xc_pairs: weights of shape {tuple(h.shape)}, expected (2, >= {ncomp}, {ng})")
            out.append((h[:, :ncomp], t(np.asarray([(da + da.T) * 0.5, (db + db.T) * 0.5]))))
        return out
    return _grad_xc_run(mf, items, chunk, stats)


def _grad_xc_run(mf, make_items, chunk, stats):
    """The chunk loop of ``grad_xc_device`` / ``grad_xc_pairs`` over the (h, densities) items that
    ``make_items(engine, to_device)`` returns."""
    import torch
    from .dints import _sph_table, ao_shell_tables
    eng = getattr(mf, "device_engine", None)
    if eng is None or mf.xctype not in ("LDA", "GGA"):
        raise RuntimeError("grad_xc_device needs a built LDA / GGA mean field on a device (mf.to_device())")
    mol = mf.mol
    gga = mf.xctype == "GGA"
    L = _capi.lib()
    dv = eng.dev
    n, natm, nshell = mol.nao, mol.natm, len(mol.shells)
    ng = int(eng.w.shape[0])
    chunk = default_xc_chunk(n, ng) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    info, dat = ao_shell_tables(mol)
    with torch.cuda.device(dv):
        def t(x):
            return torch.as_tensor(np.ascontiguousarray(x), device=dv)
        items = make_items(eng, t)
        coords = t(np.asarray(mf.grids.coords, dtype=np.float64))
        t_info, t_dat, t_sph, t_nrm = t(info), t(dat), t(_sph_table()), t(mol._norm)
        t_atom = t(np.array([s.atom for s in mol.shells], dtype=np.int32))
        lmax = max(s.l for s in mol.shells)
        out = torch.zeros((natm, 3), dtype=torch.float64, device=dv)
        nwork = xc_work_size(min(chunk, ng), nshell)
        work = torch.empty(nwork, dtype=torch.float64, device=dv)
        st = ctypes.c_void_p(torch.cuda.current_stream(dv).cuda_stream)
        ao = eng.ao
        tg = tk = 0.0
        nbytes = 0
        for h, dms in items:
            for g0 in range(0, ng, chunk):
                g1 = min(ng, g0 + chunk)
                m = g1 - g0
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    t0 = time.perf_counter()
                hc = torch.zeros((2, 4, m), dtype=torch.float64, device=dv)
                hc[:, :h.shape[1]] = h[:, :, g0:g1]
                a0 = ao[0, g0:g1]
                e = torch.empty((2, n, m), dtype=torch.float64, device=dv)
                c = torch.empty((2, n, m), dtype=torch.float64, device=dv) if gga else None
                for s in range(2):
                    b = hc[s, 0][:, None] * a0
                    if gga:
                        for k in range(1, 4):
                            b = b + hc[s, k][:, None] * ao[k, g0:g1]
                        eng._gemm(0, 1, n, m, n, 1.0, dms[s], n, a0, n, 0.0, c[s], m)       # c_s^T = D_s phi^T
                    eng._gemm(0, 1, n, m, n, 1.0, dms[s], n, b.contiguous(), n, 0.0, e[s], m)   # e_s^T = D_s b_s^T
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    tg += time.perf_counter() - t0
                    t0 = time.perf_counter()
                _capi.check(L.xt_grad_xc(m, coords[g0:g1].data_ptr(), nshell, t_info.data_ptr(), t_dat.data_ptr(),
                                         t_sph.data_ptr(), t_nrm.data_ptr(), t_atom.data_ptr(), lmax, natm, n, 2,
                                         _capi.XC["GGA" if gga else "LDA"], hc.data_ptr(), e.data_ptr(),
                                         c.data_ptr() if gga else None, m, work.data_ptr(), nwork, out.data_ptr(), st),
                            "xt_grad_xc")
                if stats is not None:
                    torch.cuda.synchronize(dv)
                    tk += time.perf_counter() - t0
                    nbytes += 8 * m * (2 * n * (2 if gga else 1) + (6 if gga else 0))
        if stats is not None:
            stats.update(gemm_s=tg, grad_xc_s=tk, grad_xc_bytes=nbytes, chunk=chunk, ngrid=ng,
                         chunks=(ng + chunk - 1) // chunk)
        return -2.0 * out.cpu().numpy()


def ks_ground_terms(d0a, d0b, hyb):
    """The kernel terms of the UKS two-electron gradient: J[D_a + D_b] with D_a + D_b and, for a
    hybrid, -hyb K[D_s] with D_s per spin; a pure functional is the J term alone, so
    ``xt_grad_jk`` forms no exchange contraction.  A range-separated functional takes the terms of
    hyb = 1 through ``pair_lists`` and ``grad_jk_rsh``, which weights the exchange pairs per operator."""
    d0t = d0a + d0b
    terms = [jk_terms(1, 0, d0t, d0t)]
    if hyb != 0:
        terms += [jk_terms(0, -hyb, d0a, d0a), jk_terms(0, -hyb, d0b, d0b)]
    return terms


def check_ks_gradient_mf(mf, *, allow_rsh=False):
    """The Kohn-Sham mean fields ``KSGradients`` covers: unrestricted, LDA or GGA (pure or global
    hybrid), exact integrals, no non-local correlation.  ``allow_rsh``: range-separated hybrids pass
    (the ``.Gradients()`` doors; ``nuc_grad_method()`` keeps refusing them)."""
    if getattr(mf, "restricted_open", False):
        raise NotImplementedError("nuclear gradients need a UKS reference: an ROKS determinant is not "
                                  "variational in the rotations the formula assumes")
    xc = str(getattr(mf, "xc", "HF"))
    xctype = _xc.xc_type(xc) if xc.upper() != "HF" else "HF"
    if xctype == "HF":
        raise NotImplementedError("KSGradients is for Kohn-Sham mean fields; Hartree-Fock has qc.grad.Gradients")
    if xctype == "MGGA":
        raise NotImplementedError(f"nuclear gradients for the meta-GGA {xc!r}: the tau derivative of the XC "
                                  "potential is not built (LDA / GGA only)")
    if xctype not in ("LDA", "GGA"):
        raise NotImplementedError(f"nuclear gradients for xc = {xc!r} of type {xctype}")
    if _xc.rsh_and_hybrid_coeff(xc)[0] != 0 and not allow_rsh:
        raise NotImplementedError(f"nuclear gradients for the range-separated {xc!r}: xt_grad_jk has no "
                                  "long-range (erf) operator; xt_grad_jk2_lr has, and the gradient comes from "
                                  "the .Gradients() entry of the same object (nuc_grad_method() stays as it was)")
    if getattr(mf, "nlc", None) is not None:
        raise NotImplementedError("nuclear gradients with VV10 non-local correlation: its derivative is not built")
    _check_exact_integrals(mf)


class KSGradients(Gradients):
    """``UKS.nuc_grad_method()`` after ``to_device()``: the one-electron and overlap terms with the
    energy-weighted density of the Kohn-Sham Fock matrix, J - hyb K through ``xt_grad_jk`` and the
    XC term through ``xt_grad_xc``.  The grid does not move with the nuclei (``grid_response`` is
    False and cannot be switched on): the result is the exact derivative of the energy on a grid
    whose points and weights are held fixed, and it differs from the derivative on an
    atom-centred grid by the weight derivatives, which vanish with the grid error."""

    def __init__(self, mf, *, allow_rsh=False):
        self._allow_rsh = allow_rsh
        super().__init__(mf)
        self.de_xc = None        # the XC part of the last gradient, (natm, 3)
        self.xc_chunk = None     # grid points per xt_grad_xc call; None: default_xc_chunk

    def _check_mf(self, mf):
        check_ks_gradient_mf(mf, allow_rsh=self._allow_rsh)

    def _device(self):
        dev = super()._device()
        if getattr(self.base, "device_engine", None) is None:
            raise RuntimeError("the XC gradient runs on the GPU (xt_grad_xc): run the SCF after mf.to_device()")
        return dev

    @property
    def grid_response(self):
        return False

    @grid_response.setter
    def grid_response(self, on):
        if on:
            raise NotImplementedError("grid_response = True: the derivatives of the grid weights are not built")

    def grad_elec(self, atmlst=None):
        mf = self.base
        dev, d0a, d0b, de = self._one_electron()
        omega = float(getattr(mf, "omega", 0.0))
        # range-separated, hyb K + (alpha - hyb) K_LR: the pairs of full exchange, weighted once per operator
        rsh = (omega, float(mf.alpha)) if omega != 0 else None
        terms = ks_ground_terms(d0a, d0b, mf.hyb if rsh is None else 1.0)
        de += grad_2e(self.mol, dev, self.timings, float(mf.hyb), rsh, terms=terms)
        t0 = time.perf_counter()
        sx = {}
        self.de_xc = grad_xc_device(mf, d0a, d0b, chunk=self.xc_chunk, stats=sx)
        de += self.de_xc
        self.timings["grad_xc_call_s"] = time.perf_counter() - t0
        self.timings.update(sx)
        return de if atmlst is None else de[list(atmlst)]
