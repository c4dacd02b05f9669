"""Spin-orbit state interaction between the three TDA manifolds of a high-spin ROKS reference
(``SI_driver``, x2c_hamiltonian/driver/si_driver.py, as x2c_hamiltonian/test_SOCSI.py runs it).

From a mean-field spin-orbit operator ``Vso`` (3, nmo, nmo), real antisymmetric in the MO
basis, and the roots |S-1> (``XSF_TDA``), |S> (``XTDA``) and |S+1> (``SF_TDA_up``), the
driver builds the reduced matrix elements <Psi_L||h||Psi_R> of every pair of states, expands
them over M with the Wigner-Eckart factor into H_eff = Omega + h_so, diagonalises it on the
host and reports the spin-orbit levels and the moments between them.

The reduced elements are bilinear in the two states and linear in the operator with real
factors, so the device entry ``xt_si_couple`` (``include/xtddft_amd.h``) evaluates them for
all pairs at once on the three real components of ``Vso`` (``si_couple``); the host forms
h^m = (-i V_x - V_y, i sqrt(2) V_z, i V_x - V_y), the reference's reversed ``hm[..., ::-1]``,
from the three results.  The reference loops over the pairs in Python instead.

Index convention (si_driver.py:329-391): groups in the order |S->, |GS>, |So>, |S+>;
position = group offset + M_index n_group + i with M_index = M + S_group.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _capi
from .utils import HA2EV, so2st as _so2st

EV2CM_1 = 8065.544005          # xtddft/utils/unit.py
AU2DEBYE = 2.541746473
SQRT2 = math.sqrt(2.0)
GROUPS = ('|S->', '|GS>', '|So>', '|S+>')     # the order of H_eff's blocks
# h^m, m = 0, 1, 2 over the components (x, y, z) of Vso: cal_hm's hm[..., ::-1]
HM = np.array([[-1j, -1.0, 0.0], [0.0, 0.0, 1j * SQRT2], [1j, -1.0, 0.0]])


# ---- Wigner-Eckart factor ----------------------------------------------------
def _twice(x, what):
    t = round(2 * float(x))
    if abs(2 * float(x) - t) > 1e-8:
        raise ValueError(f"{what} must be an integer or a half-integer, got {x}")
    return int(t)


def _f(n2):
    """(n2 / 2)! for an even, non-negative doubled argument."""
    return math.factorial(n2 // 2)


def threej_rank1(j1, m1, m2, j3, m3):
    """The 3j symbol (j1 1 j3; m1 m2 m3) by Racah's closed form (at most three terms for
    rank 1); arguments doubled (integers).  0 outside the triangle / projection rules."""
    j2 = 2
    if m1 + m2 + m3 != 0 or j1 < 0 or j3 < 0:
        return 0.0
    if abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3:
        return 0.0
    if (j1 + m1) % 2 or (j3 + m3) % 2 or (j2 + m2) % 2 or (j1 + j2 + j3) % 2:
        return 0.0
    if j3 > j1 + j2 or j3 < abs(j1 - j2):
        return 0.0
    delta = _f(j1 + j2 - j3) * _f(j1 - j2 + j3) * _f(-j1 + j2 + j3) / _f(j1 + j2 + j3 + 2)
    norm = (_f(j1 + m1) * _f(j1 - m1) * _f(j2 + m2) * _f(j2 - m2) * _f(j3 + m3) * _f(j3 - m3))
    total = 0.0
    for t in range(0, j1 + j2 - j3 + 1, 2):          # doubled t
        args = (t, j3 - j2 + t + m1, j3 - j1 + t - m2, j1 + j2 - j3 - t, j1 - t - m1, j2 - t + m2)
        if min(args) < 0:
            continue
        den = 1.0
        for a in args:
            den *= _f(a)
        total += (-1.0) ** (t // 2) / den
    return (-1.0) ** ((j1 - j2 - m3) // 2) * math.sqrt(delta * norm) * total


def w(S, M, Sp, Mp):
    """w(S, M, S', M') = (-1)^(S-M) (S 1 S'; -M, M-M', M') / (S 1 S'; -S, S-S', S')
    (si_driver.py:46-65) in closed form; 0 where the denominator vanishes."""
    s, m, sp, mp = _twice(S, "S"), _twice(M, "M"), _twice(Sp, "S'"), _twice(Mp, "M'")
    if (s - m) % 2:
        raise ValueError(f"S - M must be an integer, got {(s - m) / 2}")
    den = threej_rank1(s, -s, s - sp, sp, sp)
    if abs(den) < 1e-9:
        return 0.0
    phase = -1.0 if ((s - m) // 2) % 2 else 1.0
    return phase * threej_rank1(s, -m, m - mp, sp, mp) / den


# ---- the device call ---------------------------------------------------------
def si_couple(op_mo, s, nc, no, nv, x_sm=None, x_so=None, x_sp=None, with_ground=True, mode="soc", device=0):
    """(ncomp, n, n) couplings of the real MO operator ``op_mo`` (ncomp, nmo, nmo) between
    the states in the rows of ``x_sm`` / ``x_so`` / ``x_sp`` (the reference's layouts) and the
    reference state, n = n_sm + with_ground + n_so + n_sp in the group order of H_eff
    (``xt_si_couple``).  ``mode`` 'soc': antisymmetric operator, the rank-1 tables of
    si_driver.py; same-manifold blocks in full and the blocks with L before R.  'dipole':
    symmetric operator, the same-S blocks of tdm.py."""
    import torch
    op_mo = np.ascontiguousarray(op_mo, dtype=np.float64)
    nmo = nc + no + nv
    if op_mo.ndim != 3 or op_mo.shape[1:] != (nmo, nmo):
        raise ValueError(f"operator has shape {op_mo.shape}, expected (ncomp, {nmo}, {nmo})")
    cv, co, ov = nc * nv, nc * no, no * nv
    dims = (cv + co + ov + no * no + no, 2 * cv + co + ov, cv)
    xs = []
    for x, dim, name in zip((x_sm, x_so, x_sp), dims, ('|S->', '|So>', '|S+>')):
        x = np.zeros((0, dim)) if x is None else np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != dim:
            raise ValueError(f"{name} vectors have shape {x.shape}, expected (n, {dim})")
        xs.append(x)
    g = int(bool(with_ground))
    n = xs[0].shape[0] + g + xs[1].shape[0] + xs[2].shape[0]
    d = _capi.XtSiDesc(nc=nc, no=no, nv=nv, ncomp=op_mo.shape[0], s=float(s), n_sm=xs[0].shape[0],
                       n_so=xs[1].shape[0], n_sp=xs[2].shape[0], with_ground=g, mode=_capi.SI_MODE[mode])
    out = np.empty((op_mo.shape[0], n, n))
    L = _capi.lib()
    dev = torch.device(f"cuda:{device}")
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(L.xt_si_couple(ctypes.byref(d), op_mo.ctypes.data, *(x.ctypes.data if x.size else None for x in xs),
                                   out.ctypes.data, _capi.XT_PTR_HOST, ctypes.c_void_p(st)), "xt_si_couple")
    return out


# ---- the three producers ------------------------------------------------------
def states_from_xsf(xsf):
    """[(e, X)] in the |S-> layout [CV(1) | CO(1) | OV(1) | O1O2 | O1O1] from the roots of an
    ``XSF_TDA`` (test_SOCSI.py:42-70): a compressed OO block is expanded with ``xsf.vects``
    and split into its off-diagonal part (O1O2, zero diagonal) and its diagonal (O1O1)."""
    nc, no, nv = xsf.nc, xsf.no, xsf.nv
    v = np.asarray(xsf.v)
    d3 = nc * nv + nc * no + no * nv
    oo = xsf.vects @ v[d3:] if getattr(xsf, "re", False) else v[d3:]
    if oo.shape[0] != no * no or v.shape[0] - (no * no - oo.shape[0]) < d3:
        raise ValueError("the roots do not span the full cv|co|ov|oo space (frozen core?)")
    n = v.shape[1]
    oo = oo.reshape(no, no, n)
    diag = np.einsum('iin->in', oo)
    off = oo - np.einsum('in,ij->ijn', diag, np.eye(no))
    x = np.concatenate([v[:d3], off.reshape(no * no, n), diag], axis=0)
    return [(float(xsf.e[i]), np.ascontiguousarray(x[:, i])) for i in range(n)]


def states_from_sf_up(sf):
    """[(e, X)] in the |S+> layout CV(1) (nc x nv) from the roots of an ``SF_TDA_up``
    (test_SOCSI.py:88-103)."""
    if getattr(sf, "isf", 0) != 1:
        raise ValueError("states_from_sf_up needs a spin-flip-up solver")
    n = sf.nstates
    v = np.asarray(sf.v)[:, :n]
    if v.shape[0] != sf.nc * sf.nv:
        raise ValueError(f"spin-flip-up vectors have length {v.shape[0]}, expected nc nv = {sf.nc * sf.nv}")
    return [(float(sf.e[i]), np.ascontiguousarray(v[:, i])) for i in range(v.shape[1])]


def states_from_xtda(xtda):
    """[(e, X)] in the |So> layout [CV(0) | CO(0) | OV(0) | CV(1)] from the roots of an X-TDA
    ``XTDA`` on a ROKS reference: "my order" through ``utils.so2st`` and the block reorder.
    CV(1) changes sign: tdm.py's TDM_S and si_driver.py assume the phase opposite to so2st's
    (``xt_tdm_sc``: -sqrt((S+1)/(2S)) in so2st's phase where tdm.py writes +)."""
    if not getattr(xtda, "X", False):
        raise ValueError("state interaction needs the X-TDA roots of a ROKS reference")
    nc, no, nv = xtda.nc, xtda.no, xtda.nv
    st = _so2st(np.asarray(xtda.v), nc, no, nv)          # [cv0 | ov0 | co0 | cv1]
    cv, ov = nc * nv, no * nv
    x = np.concatenate([st[:cv], st[cv + ov:cv + ov + nc * no], st[cv:cv + ov], -st[cv + ov + nc * no:]], axis=0)
    return [(float(xtda.e[i]), np.ascontiguousarray(x[:, i])) for i in range(x.shape[1])]


def symm_matrix(h):
    """The upper triangle and its Hermitian image below it (si_driver.py:67-71)."""
    return np.triu(h) + np.triu(h, 1).T.conjugate()


class SI_driver:
    """``SI_driver(mf, S, Vso, ngs=1, states={...}, cal_osc=False)`` (si_driver.py:75-125).

    ``states`` maps '|S->', '|So>', '|S+>' to lists of ``(e, X)``; ``ngs=1`` adds the
    reference state ``(0.0, [1.0])``.  ``Vso`` (3, nmo, nmo) real antisymmetric in the MO
    basis.  With ``cal_osc`` the dipole integrals come from ``dipole_ao`` (3, nao, nao), by
    default ``int1e_r`` at the centre of nuclear charge of a Mole with integrals, and the
    reference state's own moment from ``ref_dipole`` (default: -tr(r D) of the default
    integrals; zero when ``dipole_ao`` is given without it)."""

    def __init__(self, mf=None, S=None, Vso=None, ngs=1, states=None, cal_osc=False, device=0,
                 dipole_ao=None, ref_dipole=None):
        self.mf = mf
        self.mol = mf.mol
        self.cal_osc = bool(cal_osc)
        self.device = device
        self.couple = si_couple          # the device call (the host tests put the restatement here)
        self.S = float(S)
        _twice(self.S, "S")
        if self.S != self.mol.spin / 2.0:
            raise ValueError(f"S = {S} is not the reference's mol.spin / 2 = {self.mol.spin / 2.0}")
        self.str2S = {'|GS>': self.S, '|So>': self.S, '|S+>': self.S + 1, '|S->': self.S - 1}
        self.S2str = {(self.S, 1): '|GS>', (self.S, 0): '|So>', (self.S + 1, 0): '|S+>', (self.S - 1, 0): '|S->'}
        self.ngs = int(ngs)
        if self.ngs not in (0, 1):
            raise ValueError("ngs must be 0 or 1")
        self.states = dict(states or {})
        unknown = set(self.states) - set(GROUPS)
        if unknown:
            raise ValueError(f"unknown state labels {sorted(unknown)}; expected '|S->', '|So>', '|S+>'")
        self.states['|GS>'] = [(0.0, np.array([1.0]))] if self.ngs else []
        for k in GROUPS:
            self.states[k] = list(self.states.get(k, []))
        self.cal_dims()
        Vso = np.asarray(Vso, dtype=np.float64) if Vso is not None else None
        if Vso is None or Vso.shape != (3, self.norb, self.norb):
            raise ValueError(f"Vso must be (3, {self.norb}, {self.norb}) in the MO basis")
        if not np.allclose(Vso, -Vso.transpose(0, 2, 1), rtol=0.0, atol=1e-10 * max(1.0, np.abs(Vso).max())):
            raise ValueError("Vso must be real antisymmetric in the MO basis")
        self.Vso = Vso
        self.hm = self.cal_hm(Vso)
        self._vectors()
        if self.cal_osc:
            self.ints_mo = self.cal_edm_mu(dipole_ao, ref_dipole)

    # ---- setup -----------------------------------------------------------------
    def cal_hm(self, Vso):
        """(nmo, nmo, 3) complex h^m in the reversed order of si_driver.py:228-238."""
        return np.einsum('mk,kpq->pqm', HM, Vso)

    def cal_edm_mu(self, dipole_ao, ref_dipole):
        from . import tdm as _tdm
        default = dipole_ao is None
        if default:
            dipole_ao = _tdm.charge_centre_dipole(self.mf, self.mol)
        dipole_ao = np.asarray(dipole_ao, dtype=np.float64)
        c = np.asarray(self.mf.mo_coeff)
        if c.ndim != 2:
            raise ValueError("state interaction needs a ROKS / RKS reference (one set of orbitals)")
        if ref_dipole is None:
            # the nuclear part vanishes at the centre of nuclear charge
            ref_dipole = -np.einsum('xpq,spq->x', dipole_ao, self.mf.make_rdm1()) if default else np.zeros(3)
        self.mu_nuc = np.asarray(ref_dipole, dtype=np.float64)
        return np.einsum('xpq,pi,qj->xij', dipole_ao, c, c)

    def cal_dims(self):
        mol = self.mol
        if hasattr(self.mf, "shape_info"):
            info = self.mf.shape_info()
            self.norb = info['nmo']
            nc, no, nv = info['nc'], info['no'], info['nv']
        else:
            self.norb = mol.nao
            no = int(round(2 * self.S))
            nc = (mol.nelectron - no) // 2
            nv = self.norb - nc - no
        if no != int(round(2 * self.S)) or min(nc, no, nv) < 0:
            raise ValueError("the orbital counts do not describe a high-spin reference of spin S")
        self.n = self.nc, self.no, self.nv = nc, no, nv
        self.cv, self.co, self.ov, self.oo = nc * nv, nc * no, no * nv, no * no
        self.dim_Sm = self.cv + self.co + self.ov + self.oo + no
        self.dim_So = self.cv + self.co + self.ov + self.cv
        self.dim_Sp = self.cv
        self.nGS = self.ngs
        self.nSo, self.nSp, self.nSm = (len(self.states[k]) for k in ('|So>', '|S+>', '|S->'))
        if self.nSm and self.S < 1:
            raise ValueError("|S-> states need a reference with S >= 1")
        s2 = int(round(2 * self.S))
        mult = {'|S->': max(s2 - 1, 0), '|GS>': s2 + 1, '|So>': s2 + 1, '|S+>': s2 + 3}
        self.str2nS = {'|S->': self.nSm, '|GS>': self.nGS, '|So>': self.nSo, '|S+>': self.nSp}
        self.str2dim, off = {}, 0
        for k in GROUPS:
            self.str2dim[k] = off
            off += mult[k] * self.str2nS[k]
        self.dim0, self.dim1, self.dim2 = (self.str2dim[k] for k in ('|GS>', '|So>', '|S+>'))
        self.dim3 = self.dim_hso = off
        self._mult = mult

    def _vectors(self):
        """The state vectors of each manifold as rows; lengths checked."""
        def rows(key, dim, short=None):
            out = np.zeros((len(self.states[key]), dim))
            for i, (_, x) in enumerate(self.states[key]):
                x = np.asarray(x, dtype=np.float64).ravel()
                if x.size == dim:
                    out[i] = x
                elif short is not None and x.size == short:
                    out[i, :short] = x
                else:
                    raise ValueError(f"{key} vector {i} has length {x.size}, expected {dim}")
            return out
        self.x_sm = rows('|S->', self.dim_Sm)
        # a closed-shell |So> vector may come without its CV(1) block (reformat_S, si_driver.py:928-942)
        self.x_so = rows('|So>', self.dim_So, self.cv + self.co + self.ov if self.S == 0 else None)
        self.x_sp = rows('|S+>', self.dim_Sp)

    # ---- index convention ----------------------------------------------------------
    def cal_hso_pos(self, SL, ML, Li, igsL, SR, MR, Ri, igsR, debug=0):
        """(row, column) of <SL ML Li|h|SR MR Ri> in H_eff (si_driver.py:329-358)."""
        kl, kr = self.S2str[(SL, igsL)], self.S2str[(SR, igsR)]
        return (int(self.str2dim[kl] + (ML + SL) * self.str2nS[kl] + Li),
                int(self.str2dim[kr] + (MR + SR) * self.str2nS[kr] + Ri))

    def cal_pos(self, pos):
        """(S, M, i, igs) of a position in H_eff (si_driver.py:368-391)."""
        if not 0 <= pos < self.dim_hso:
            raise ValueError(f"position {pos} outside H_eff of dimension {self.dim_hso}")
        for k in reversed(GROUPS):
            if pos >= self.str2dim[k] and self._mult[k] * self.str2nS[k] > 0:
                m, ith = divmod(pos - self.str2dim[k], self.str2nS[k])
                S = self.str2S[k]
                return (S, -S + m, ith, int(k == '|GS>'))
        raise ValueError(f"position {pos} missing")

    def cal_pos_hso(self, L_pos, R_pos):
        return (*self.cal_pos(L_pos), *self.cal_pos(R_pos))

    def _slots(self, key):
        """[(M, first position)] of a group."""
        S, n = self.str2S[key], self.str2nS[key]
        return [(-S + k, self.str2dim[key] + k * n) for k in range(self._mult[key])] if n else []

    # ---- H_eff -----------------------------------------------------------------------
    def reduced_elements(self):
        """(3, n, n) complex <Psi_L||h^m||Psi_R> without the geometric factor, from the three
        real component results of the device call: upper blocks only (``make_hso_local``)."""
        c = self.couple(self.Vso, self.S, self.nc, self.no, self.nv, self.x_sm, self.x_so, self.x_sp,
                        with_ground=bool(self.ngs), mode="soc", device=self.device)
        return np.einsum('mk,kij->mij', HM, c)

    def make_heff(self):
        """H_eff = Omega + h_so (si_driver.py:393-470): the upper triangle from the reduced
        elements and w, Hermitian completion, zero diagonal of h_so, Omega on the diagonal."""
        h = self.reduced_elements()
        first, k0 = {}, 0
        for k in GROUPS:
            first[k] = k0
            k0 += self.str2nS[k]
        dim = self.dim_hso
        hso = np.zeros((dim, dim), dtype=np.complex128)
        Omega = np.zeros((dim, dim))
        for a, kl in enumerate(GROUPS):
            nl, SL = self.str2nS[kl], self.str2S[kl]
            e = np.array([s[0] for s in self.states[kl]], dtype=np.float64)
            for _, p in self._slots(kl):
                Omega[np.arange(p, p + nl), np.arange(p, p + nl)] = e
            for kr in GROUPS[a:]:
                nr, SR = self.str2nS[kr], self.str2S[kr]
                if abs(SR - SL) > 1:
                    continue
                blk = h[:, first[kl]:first[kl] + nl, first[kr]:first[kr] + nr]
                for ML, pl in self._slots(kl):
                    for MR, pr in self._slots(kr):
                        if abs(MR - ML) <= 1:
                            hso[pl:pl + nl, pr:pr + nr] = blk[int(MR - ML) + 1] * w(SL, ML, SR, MR)
        self.hso = symm_matrix(hso)
        self.hso = self.hso - np.diag(np.diag(self.hso))
        self.Omega = Omega
        self.heff = self.hso + self.Omega
        if self.cal_osc:
            self.dm = self.make_dm(first)
        return self.heff

    def make_dm(self, first):
        """(dim, dim, 3) moments between the basis states: the same-(S, M) blocks of the
        dipole couplings, the reference state's own moment on the diagonal
        (si_driver.py:416-459, 871-916)."""
        d = self.couple(self.ints_mo, self.S, self.nc, self.no, self.nv, self.x_sm, self.x_so, self.x_sp,
                        with_ground=bool(self.ngs), mode="dipole", device=self.device)
        dim = self.dim_hso
        dm = np.zeros((dim, dim, 3))
        for kl, kr in (('|S->', '|S->'), ('|GS>', '|So>'), ('|So>', '|So>'), ('|S+>', '|S+>')):
            nl, nr = self.str2nS[kl], self.str2nS[kr]
            blk = d[:, first[kl]:first[kl] + nl, first[kr]:first[kr] + nr].transpose(1, 2, 0)
            for (_, pl), (_, pr) in zip(self._slots(kl), self._slots(kr)):
                dm[pl:pl + nl, pr:pr + nr, :] = blk
        for x in range(3):
            dm[..., x] = symm_matrix(dm[..., x])
        dm[np.arange(dim), np.arange(dim), :] += self.mu_nuc
        return dm

    def kernel(self, printnum=100):
        """Diagonalise H_eff; returns ``(eso, vso)`` and sets ``heff``, ``hso``, ``Omega``,
        ``esf`` and, with ``cal_osc``, ``dm`` and ``dmso`` (si_driver.py:127-154)."""
        import scipy.linalg
        self.make_heff()
        self.eso, self.vso = scipy.linalg.eigh(self.heff, driver='evd')
        if self.cal_osc:
            # V^+ dm V per component (the reference's einsum string 'ij,ikn,kl->iln' contracts
            # neither index of V^+ with dm; the transformation it describes is this one)
            self.dmso = np.einsum('ij,ikn,kl->jln', self.vso.conjugate(), self.dm, self.vso)
        self.esf = np.einsum('ij,i,ij->j', self.vso.conjugate(), np.diag(self.Omega), self.vso).real
        if printnum:
            self.summary(printnum)
        return self.eso, self.vso

    # ---- reports ---------------------------------------------------------------------
    def v2state(self, v):
        """The label of an eigenvector's largest component and that state's spin-free
        energy (si_driver.py:212-226)."""
        v2 = (v.conjugate() * v).real
        pos = int(np.argmax(v2))
        S, M, ith, igs = self.cal_pos(pos)
        strS = self.S2str[(S, igs)]
        state_str = f'{ith:>3d}-th   ' + strS[:-1] + f', {M:+.1f}⟩      {100 * v2[pos]:>5.1f}%'
        return state_str, self.states[strS][ith][0]

    def summary(self, printnum=100):
        print(f"|Ref⟩ with S = Sz = {self.S}, E = {getattr(self.mf, 'e_tot', 0.0)} Hartree")
        print(f"Interaction among {self.nSm} |S-⟩, {self.ngs} |GS⟩, {self.nSo} |So⟩, {self.nSp} |S+⟩.")
        print("  No   i-th   Excited state    v**2        Esf(eV)       Eso(eV)     En-E1(eV)    En-E1(cm-1)")
        for i, e in enumerate(self.eso[:printnum]):
            label, e_sf = self.v2state(self.vso[:, i])
            de = (e - self.eso[0]) * HA2EV
            print(f"{i:4d} {label}  {e_sf * HA2EV:>12.8f}  {e * HA2EV:>12.8f}     {de:>10.8f}    {de * EV2CM_1:>10.2f}")

    def summary_osc(self, printnum=100, unit='eV'):
        n = min(printnum, len(self.eso))
        for i in range(n):
            for j in range(n):
                self.print_osc_local(i, j, unit)

    def print_osc_local(self, i, j, unit_='eV'):
        """dE and f = (2/3) dE |r_ij|^2 between spin-orbit levels i and j (si_driver.py:175-192)."""
        if not self.cal_osc:
            raise ValueError("You must set `cal_osc=True` to calculate Dipole moments and Oscillator strength!")
        scale = {'au': 1.0, 'eV': HA2EV, 'debye': AU2DEBYE}[unit_]
        dm = self.dmso[i, j, :]
        dE = self.eso[j] - self.eso[i]
        dmu = dm.conjugate() @ dm
        f = ((2 / 3) * dE * dmu).real
        print(f'\n[{i:>3d}] <--- [{j:>3d}]: |rij|**2={dmu.real:<10.8f}, △E = {dE * scale:>10.8f} {unit_}, f = {f:<10.8f}')
        print("                          X           Y           Z")
        print(f"              Real   {dm[0].real:>8.4f}    {dm[1].real:>8.4f}    {dm[2].real:>8.4f}")
        print(f"              Imag   {dm[0].imag:>8.4f}    {dm[1].imag:>8.4f}    {dm[2].imag:>8.4f}")
        print('-' * 50)
        return dE, f

    def print_hso_local(self, SML, SMR):
        """One element of h_so by its quantum numbers (S, M, i, igs) (si_driver.py:194-202)."""
        SL, ML, iL, igsL = SML
        SR, MR, iR, igsR = SMR
        strL, strR = self.S2str[(SL, igsL)], self.S2str[(SR, igsR)]
        marker = '⟨' + strL[1:-1] + f" {ML:.1f} {iL}|hso|" + strR[1:-1] + f" {MR:.1f} {iR}⟩"
        hso = self.hso[self.cal_hso_pos(SL, ML, iL, igsL, SR, MR, iR, igsR)]
        print(f"{marker} = {hso:.8f} Ha. = {hso * HA2EV:.8f} eV = {hso * HA2EV * EV2CM_1:.8f} cm-1")
        return hso

    def print_hso(self):
        for lp in range(self.dim_hso):
            for rp in range(lp, self.dim_hso):
                self.print_hso_local(self.cal_pos(lp), self.cal_pos(rp))
