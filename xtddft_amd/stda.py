"""sX-TDA / sU-TDA: the simplified open-shell TDA of ``xtddft/sTDA/os_sTDA.py`` with the
reference's API.

``OSsTDA(mol, mf, spinadapt=True, Emax=10.0, tp=1e-4, cas=True, nstates=10, union=True,
correct=False, paramtype='os')`` (os_sTDA.py:353-368) with ``kernel`` (435-1333), ``gamma``
(408-433), ``deltaS2`` (1335-1386), ``osc_str`` (1388-1418) and ``rot_str`` (1420-1468).

The host forms the Fock matrices, chooses the CAS window, builds S^1/2 and the gamma matrices
(O(nao^3) and O(natm^2) set-up) and keeps the book of the CSF lists; the Loewdin charges, the
diagonal of every CSF, the perturbative selection weights and the A matrix come from the device
(``xt_stda_charges / _half / _diag / _select / _matrix``, include/xtddft_amd.h).  There is no CPU
path for those four.  ``analyze()``'s cube / molden output is not carried over.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi
from .meanfield import MeanField
from .utils import HA2EV

CGS2AU = 1 / (235.7220 * 2)    # xtddft/utils/unit.py:9 (rotatory strength a.u. -> cgs)
EIGH_MAX = 4096                # 'auto': host eigh up to this dimension, Davidson beyond
CONV_TOL = 1e-5                # Davidson residual tolerance (the project's TDA default)


def _ints(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


class OSsTDA:
    """``eta``: mapping element symbol -> chemical hardness in eV (the reference's
    ``sTDA/eta.py`` table; required, no table is shipped).  ``tp``: the selection threshold on
    the perturbative weight; the reference stores the argument but hard-codes 1e-4
    (os_sTDA.py:951), which is the default here, so the defaults agree.  ``diag``: 'eigh'
    (host ``numpy.linalg.eigh`` of A), 'davidson' (``xtddft_amd.davidson1`` on the
    device-resident A) or 'auto' (eigh up to dimension 4096).  ``Emax=None`` / 0 takes every CSF
    of the orbital space (and no CAS window, which is defined through Emax).
    ``elements`` / ``atom_coords`` (Bohr) / ``ao_atom`` (the atom of every AO, non-decreasing)
    replace what ``mol`` (an ``xtddft_amd.qc`` molecule) would provide."""

    def __init__(self, mol, mf, spinadapt=True, Emax=10.0, tp=1e-4, cas=True, nstates=10, union=True,
                 correct=False, paramtype='os', eta=None, device=0, diag='auto', elements=None,
                 atom_coords=None, ao_atom=None):
        if not isinstance(mf, MeanField):
            raise ValueError("mf must be a ROKS or UKS mean field")
        if spinadapt and not mf.is_rohf:
            raise ValueError("spinadapt=True (sX-TDA) needs a ROKS mean field")
        if not spinadapt and mf.is_rohf:
            raise ValueError("spinadapt=False (sU-TDA) needs a UKS mean field")
        if paramtype not in ('os', 'cs'):
            raise ValueError("paramtype must be 'os' or 'cs'")
        if diag not in ('auto', 'eigh', 'davidson'):
            raise ValueError("diag must be 'auto', 'eigh' or 'davidson'")
        self.mol, self.mf = mol, mf
        self.nstates, self.cas, self.spinadapt, self.Emax, self.tp = nstates, cas, spinadapt, Emax, tp
        self.union, self.correct, self.paramtype = union, correct, paramtype
        self.device, self.diag = device, diag
        self.conv_tol = CONV_TOL
        qc = self._qc_mol(required=False)
        if elements is None and qc is not None:
            elements, atom_coords, ao_atom = qc.elements, qc.atom_coords(), qc.ao_atom()
        if elements is None or atom_coords is None or ao_atom is None:
            raise ValueError("need the atoms: a Mole of xtddft_amd.qc, or elements, atom_coords and ao_atom")
        self.elements = [str(e) for e in elements]
        self.atom_coords = np.asarray(atom_coords, dtype=np.float64).reshape(len(self.elements), 3)
        ao_atom = np.asarray(ao_atom, dtype=np.int64)
        if ao_atom.size != mf.nao or np.any(np.diff(ao_atom) < 0) or ao_atom.min() < 0 or ao_atom.max() >= self.natm:
            raise ValueError("ao_atom must give every AO's atom, non-decreasing (an atom's AOs are contiguous)")
        self.ao_off = np.searchsorted(ao_atom, np.arange(self.natm + 1)).astype(np.int32)
        if eta is None:
            raise ValueError("eta (element -> chemical hardness in eV) is required")
        missing = sorted({e for e in self.elements if e not in eta})
        if missing:
            raise ValueError("eta lacks the elements " + ", ".join(missing))
        self.eta = {e: float(eta[e]) for e in set(self.elements)}

    @property
    def natm(self):
        return len(self.elements)

    def _qc_mol(self, required=True):
        mol = self.mol if hasattr(self.mol, "intor") else self.mf.extra.get("qc_mol")
        if (mol is None or not hasattr(mol, "intor")) and required:
            raise ValueError("AO property integrals need a Mole with intor (xtddft_amd.qc)")
        return mol if hasattr(mol, "intor") else None

    # ------------------------------------------------------------------ set-up on the host
    def gamma(self, hyb):
        """(gamma_j, gamma_k), OSsTDA.gamma (os_sTDA.py:408-433)."""
        d = self.atom_coords[:, None, :] - self.atom_coords[None, :, :]
        r = np.sqrt((d * d).sum(axis=2))
        eta = np.array([2.0 * self.eta[e] / HA2EV for e in self.elements])
        eta = (eta[:, None] + eta[None, :]) / 2
        if self.paramtype == 'cs':
            beta = 0.20 + hyb * 1.83
            gj = (1. / (r ** beta + (hyb * eta) ** (-beta))) ** (1. / beta)
        else:
            beta = hyb + 0.3
            gj = (1. / (r ** beta + (1.4 * hyb * eta) ** (-beta))) ** (1. / beta)
        alpha = 1.42 + hyb * 0.48
        gk = (1. / (r ** alpha + eta ** (-alpha))) ** (1. / alpha)
        return gj, gk

    def _window(self, occ, energy, hyb):
        """Active orbitals [lo, hi] (os_sTDA.py:504-548)."""
        nmo = occ.shape[1]
        if not (self.cas and self.Emax):
            return 0, nmo - 1
        open_ = np.flatnonzero(occ[0] != occ[1])
        if open_.size == 0:
            raise ValueError("cas=True needs open shells: the window is measured from them")
        first, last = open_[0], open_[-1]
        reach = 2 * (1. + 0.8 * hyb) * self.Emax / HA2EV
        below = [int(np.sum((energy[s] < energy[s, first]) & (energy[s] > energy[s, first] - reach))) for s in (0, 1)]
        above = [int(np.sum((energy[s] > energy[s, last]) & (energy[s] < energy[s, last] + reach))) for s in (0, 1)]
        lo, hi = int(first - max(below)), int(last + max(above))
        if lo < 0 or hi >= nmo:
            raise ValueError("the orbital energies are not ordered: the CAS window leaves the orbital range")
        return lo, hi

    def _prepare(self):
        mf = self.mf
        h1e, veff = mf.get_hcore(), mf.get_veff()
        if self.spinadapt:     # the mask rule of os_sTDA.py:449-455
            c = (mf.mo_coeff, mf.mo_coeff)
            occ = np.array([(mf.mo_occ >= 1), (mf.mo_occ == 2)], dtype=np.float64)
        else:
            c = (mf.mo_coeff[0], mf.mo_coeff[1])
            occ = np.asarray(mf.mo_occ, dtype=np.float64)
        fock_ao = (h1e + veff[0], h1e + veff[1])
        if self.spinadapt:     # sorted Fock diagonals as orbital energies (os_sTDA.py:485)
            energy = np.array([np.sort(np.einsum('pi,pq,qi->i', c[s], fock_ao[s], c[s])) for s in (0, 1)])
        else:
            energy = np.asarray(mf.mo_energy, dtype=np.float64)
        lo, hi = self._window(occ, energy, mf.hyb)
        self.frozen_nc = lo
        act = slice(lo, hi + 1)
        self.mo_coeff_a, self.mo_coeff_b = c[0][:, act], c[1][:, act]
        self.occidx_a, self.viridx_a = np.where(occ[0, act] > 0.999)[0], np.where(occ[0, act] < 0.001)[0]
        self.occidx_b, self.viridx_b = np.where(occ[1, act] > 0.999)[0], np.where(occ[1, act] < 0.001)[0]
        nocc = (len(self.occidx_a), len(self.occidx_b))
        nvir = (len(self.viridx_a), len(self.viridx_b))
        for s, idx in enumerate((self.occidx_a, self.occidx_b)):
            if not np.array_equal(idx, np.arange(nocc[s])):
                raise ValueError("the occupied orbitals must come first in the active window")
        self.nc, self.no, self.nv = nocc[1], nocc[0] - nocc[1], nvir[0]
        if self.no < 0 or nvir[1] != self.no + self.nv:
            raise ValueError("need nocc_a >= nocc_b (alpha carries the open shells)")
        cs = (self.mo_coeff_a, self.mo_coeff_b)
        fock = [cs[s].T @ fock_ao[s] @ cs[s] for s in (0, 1)]
        hfock = None
        if self.spinadapt:     # ROHF-type Fock for the X term (os_sTDA.py:603-613)
            vhf = mf.get_veff_hf()
            hfock = [cs[s].T @ (h1e + vhf[s]) @ cs[s] for s in (0, 1)]
        w, u = np.linalg.eigh(mf.get_ovlp())
        if w.min() <= 0:
            raise ValueError("the AO overlap is not positive definite")
        s_half = (u * np.sqrt(w)) @ u.T
        gj, gk = self.gamma(mf.hyb)
        return nocc, nvir, fock, hfock, [s_half @ cs[0], s_half @ cs[1]], gj, gk

    # ------------------------------------------------------------------ the device side
    def _device_operands(self, nocc, nvir, fock, hfock, cprime, gj, gk):
        import torch
        L = _capi.lib()
        dev = torch.device(f"cuda:{self.device}")
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        natm = self.natm
        d = _capi.XtStdaDesc(natm=natm, nocc_a=nocc[0], nvir_a=nvir[0], nocc_b=nocc[1], nvir_b=nvir[1],
                             nc=self.nc, no=self.no, nv=self.nv, spin_adapted=int(self.spinadapt),
                             si=0.5 * self.mf.mol.spin, correct=int(bool(self.correct)),
                             delta_max=0.5 / HA2EV if self.correct else 0.0,
                             sigma_k=0.1 / HA2EV if self.correct else 0.0)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        keep, ops = [], _capi.XtStdaOps()
        g_j, g_k = up(gj), up(gk)
        _, off = _ints(self.ao_off)
        for s, tag in enumerate("ab"):
            o, v = nocc[s], nvir[s]
            cp = up(cprime[s])
            new = lambda n: torch.empty(max(n, 1), dtype=torch.float64, device=dev)
            t = dict(q_oo=new(o * o * natm), q_ov=new(o * v * natm), q_vv=new(v * v * natm),
                     k_ov=new(o * v * natm), j_vv=new(v * v * natm),
                     f_oo=up(fock[s][:o, :o]), f_vv=up(fock[s][o:, o:]))
            if hfock is not None:
                t["h_oo"], t["h_vv"] = up(hfock[s][:o, :o]), up(hfock[s][o:, o:])
            _capi.check(L.xt_stda_charges(ctypes.byref(d), s, self.mf.nao, off, cp.data_ptr(), t["q_oo"].data_ptr(),
                                          t["q_ov"].data_ptr(), t["q_vv"].data_ptr(), st), "xt_stda_charges")
            _capi.check(L.xt_stda_half(ctypes.byref(d), s, g_k.data_ptr(), g_j.data_ptr(), t["q_ov"].data_ptr(),
                                       t["q_vv"].data_ptr(), t["k_ov"].data_ptr(), t["j_vv"].data_ptr(), st),
                        "xt_stda_half")
            for name in _capi.STDA_OPS:
                if name in t:
                    setattr(ops, f"{name}_{tag}", t[name].data_ptr())
            keep.append((cp, t))
        self._dev = dict(L=L, torch=torch, dev=dev, st=st, desc=d, ops=ops, keep=(keep, g_j, g_k))

    def _diag(self, csf):
        D = self._dev
        e = D["torch"].empty(max(len(csf), 1), dtype=D["torch"].float64, device=D["dev"])
        _, p = _ints(csf)
        _capi.check(D["L"].xt_stda_diag(ctypes.byref(D["desc"]), ctypes.byref(D["ops"]), len(csf), p, e.data_ptr(),
                                        None, D["st"]), "xt_stda_diag")
        return e[:len(csf)].cpu().numpy()

    def _weights(self, csf_p, e_p, csf_n, e_n):
        D = self._dev
        t = D["torch"]
        if len(csf_n) == 0:
            return np.zeros(0)
        ep = t.as_tensor(np.ascontiguousarray(e_p), device=D["dev"]) if len(e_p) else t.empty(1, dtype=t.float64, device=D["dev"])
        en = t.as_tensor(np.ascontiguousarray(e_n), device=D["dev"])
        w = t.empty(len(csf_n), dtype=t.float64, device=D["dev"])
        _, pp = _ints(csf_p)
        _, pn = _ints(csf_n)
        _capi.check(D["L"].xt_stda_select(ctypes.byref(D["desc"]), ctypes.byref(D["ops"]), len(csf_p), pp,
                                          ep.data_ptr(), len(csf_n), pn, en.data_ptr(), w.data_ptr(), D["st"]),
                    "xt_stda_select")
        return w.cpu().numpy()

    def _matrix(self, csf):
        D = self._dev
        t, n = D["torch"], len(csf)
        free, _ = t.cuda.mem_get_info(D["dev"])
        if 8 * n * n > 0.9 * free:
            raise MemoryError(f"the A matrix of {n} CSFs ({8 * n * n / 2 ** 30:.1f} GiB) does not fit the device; "
                              f"lower Emax")
        a = t.empty((n, n), dtype=t.float64, device=D["dev"])
        _, p = _ints(csf)
        _capi.check(D["L"].xt_stda_matrix(ctypes.byref(D["desc"]), ctypes.byref(D["ops"]), n, p, a.data_ptr(), D["st"]),
                    "xt_stda_matrix")
        return a

    # ------------------------------------------------------------------ CSF book-keeping
    def _triples(self, cls, i, a):
        """Class-local (i, a) -> (spin, i, a) in the spin's own numbering."""
        i, a = np.asarray(i, dtype=np.int64), np.asarray(a, dtype=np.int64)
        s = np.zeros_like(i) if cls < 2 else np.ones_like(i)
        return np.stack([s, i + (self.nc if cls == 1 else 0), a + (self.no if cls == 3 else 0)], axis=1)

    def _select(self):
        """P / S selection (os_sTDA.py:682-985) on boolean class maps: returns the four final
        class-local lists."""
        nc, no, nv = self.nc, self.no, self.nv
        shapes = [(nc, nv), (no, nv), (nc, no), (nc, nv)]
        every = [np.indices(sh).reshape(2, -1) for sh in shapes]
        e_all = self._diag(np.concatenate([self._triples(k, *every[k]) for k in range(4)]))
        ends = np.cumsum([0] + [sh[0] * sh[1] for sh in shapes])
        e_cls = [e_all[ends[k]:ends[k + 1]].reshape(shapes[k]) for k in range(4)]
        pmap = [e * HA2EV <= self.Emax for e in e_cls]
        self.pcsf_before_union = (int(pmap[0].sum()), int(pmap[3].sum()))
        if self.union:     # P: union over CV(aa) / CV(bb); N: intersection = its complement
            pmap[0] = pmap[3] = pmap[0] | pmap[3]
        plist = [np.where(m) for m in pmap]
        nlist = [np.where(~m) for m in pmap]
        gather = lambda lists: (np.concatenate([self._triples(k, *lists[k]) for k in range(4)]),
                                np.concatenate([e_cls[k][lists[k]] for k in range(4)]))
        (csf_p, e_p), (csf_n, e_n) = gather(plist), gather(nlist)
        w = self._weights(csf_p, e_p, csf_n, e_n)
        self.select_weights = w
        chosen = w >= self.tp
        final, start = [], 0
        for k in range(4):
            cnt = len(nlist[k][0])
            pick = np.flatnonzero(chosen[start:start + cnt])
            start += cnt
            i = np.concatenate([plist[k][0], nlist[k][0][pick]])
            a = np.concatenate([plist[k][1], nlist[k][1][pick]])
            by_i = np.argsort(i, kind="stable")
            final.append((i[by_i], a[by_i]))
        self.scsf_before_union = tuple(len(final[k][0]) - len(plist[k][0]) for k in range(4))
        if self.union:
            both = np.zeros((nc, nv), dtype=bool)
            both[final[0]] = True
            both[final[3]] = True
            final[0] = np.where(both)
        final[3] = final[0]     # as the reference: CV(bb) takes CV(aa)'s list, with or without union (:963-965)
        self.pcsf_counts = tuple(len(x[0]) for x in plist)
        return final

    # ------------------------------------------------------------------ kernel
    def kernel(self, dipole_ao=None):
        """Returns ``(e_eV, os, rs, v)`` like the reference.  ``os`` needs AO dipole integrals:
        ``dipole_ao`` (3, nao, nao), or a molecule of ``xtddft_amd.qc``; without either it is
        None.  ``rs`` is computed for chiral molecules only (zeros otherwise)."""
        prepared = self._prepare()
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("OSsTDA runs on the GPU; no device is visible")
        # the xt_stda_* entries and xt_dgemm allocate on the CURRENT device (CSF lists, AO offsets,
        # the GEMM workspace), so `device` is made current for everything that touches the GPU
        with torch.cuda.device(self.device):
            self._solve_on_device(*prepared)
        nst = self.v.shape[1]
        if dipole_ao is None and self._qc_mol(required=False) is None:
            self.os = None
        else:
            self.os = self.osc_str(dipole_ao)
        qc = self._qc_mol(required=False)
        rs = np.zeros(nst)
        if qc is not None:
            from .qc.gto import chiral_mol
            if chiral_mol(qc):
                rs = self.rot_str()
        self.rs = rs
        self.dS2 = self.deltaS2()
        return self.e_eV, self.os, rs, self.v

    @property
    def A(self):
        """The A matrix of the selected CSFs as a host array (copied from ``A_device``, the
        device tensor both root paths keep, on first use)."""
        if self._a_host is None:
            self._a_host = self.A_device.cpu().numpy()
        return self._a_host

    def _solve_on_device(self, nocc, nvir, fock, hfock, cprime, gj, gk):
        """Operands, selection, A and the roots; runs with ``device`` current.  On both root
        paths ``e`` holds the lowest ``min(nstates, n)`` roots (Hartree) and ``v`` their vectors."""
        self._device_operands(nocc, nvir, fock, hfock, cprime, gj, gk)
        nc, no, nv = self.nc, self.no, self.nv
        if self.Emax:
            lists = self._select()
        else:
            lists = [tuple(np.indices(sh).reshape(2, -1)) for sh in [(nc, nv), (no, nv), (nc, no), (nc, nv)]]
        (self.pscsfcv_a_i, self.pscsfcv_a_a), (self.pscsfov_a_i, self.pscsfov_a_a), \
            (self.pscsfco_b_i, self.pscsfco_b_a), (self.pscsfcv_b_i, self.pscsfcv_b_a) = lists
        self.lcva, self.lova, self.lcob, self.lcvb = (len(x[0]) for x in lists)
        csf = np.concatenate([self._triples(k, *lists[k]) for k in range(4)])
        self.csf = csf
        n = len(csf)
        if n == 0:
            raise ValueError("no CSF in the space")
        a_dev = self._matrix(csf)
        nst = min(self.nstates, n)
        how = self.diag if self.diag != 'auto' else ('eigh' if n <= EIGH_MAX else 'davidson')
        self.A_device, self._a_host = a_dev, None
        if how == 'eigh':
            e, v = np.linalg.eigh(self.A)
            self.e, self.v = e[:nst], v[:, :nst]
        else:
            e, v = self._davidson(a_dev, csf, nst)
            self.e, self.v = e[:nst], v[:, :nst]
        self.nstates_found = nst
        self.e_eV = self.e * HA2EV
        ends = np.cumsum([0, self.lcva, self.lova, self.lcob, self.lcvb])
        vt = self.v.T
        self.xycv_a, self.xyov_a, self.xyco_b, self.xycv_b = (vt[:, ends[k]:ends[k + 1]] for k in range(4))

    def _davidson(self, a_dev, csf, nst):
        """Lowest roots of the device-resident A: aop is one xt_dgemm."""
        from . import davidson as _dav
        D = self._dev
        t, L, n = D["torch"], D["L"], a_dev.shape[0]
        hdiag = self._diag(csf)

        def aop(z):
            if not (hasattr(z, "is_cuda") and z.is_cuda):
                z = t.as_tensor(np.atleast_2d(np.asarray(z, dtype=np.float64)), device=D["dev"])
            z = z.contiguous()
            out = t.empty_like(z)
            st = ctypes.c_void_p(t.cuda.current_stream(D["dev"]).cuda_stream)
            _capi.check(L.xt_dgemm(0, 1, z.shape[0], n, n, 1.0, z.data_ptr(), n, a_dev.data_ptr(), n, 0.0,
                                   out.data_ptr(), n, st), "xt_dgemm")
            return out
        nguess = min(n, nst)
        x0 = np.zeros((nguess, n))
        x0[np.arange(nguess), np.argsort(hdiag, kind="stable")[:nguess]] = 1.0
        precond = _dav.DiagPrecond(hdiag, device=self.device)
        self.converged, e, x1, self.icyc = _dav.davidson1(aop, x0, precond, tol_residual=self.conv_tol, nroots=nst,
                                                          max_cycle=100, device=self.device)
        return np.asarray(e), np.asarray(x1).T

    # ------------------------------------------------------------------ properties
    def _orbital_blocks(self):
        return (self.mo_coeff_a[:, self.occidx_a], self.mo_coeff_a[:, self.viridx_a],
                self.mo_coeff_b[:, self.occidx_b], self.mo_coeff_b[:, self.viridx_b])

    def _transition(self, op_ao):
        """<0|op|n> (n, 3) of a 3-component AO operator on the selected CSFs."""
        coa, cva, cob, cvb = self._orbital_blocks()
        da = np.einsum('xpq,pi,qj->xij', op_ao, coa, cva)
        db = np.einsum('xpq,pi,qj->xij', op_ao, cob, cvb)
        return (np.einsum('xi,yi->yx', da[:, self.pscsfcv_a_i, self.pscsfcv_a_a], self.xycv_a)
                + np.einsum('xi,yi->yx', da[:, self.nc + self.pscsfov_a_i, self.pscsfov_a_a], self.xyov_a)
                + np.einsum('xi,yi->yx', db[:, self.pscsfco_b_i, self.pscsfco_b_a], self.xyco_b)
                + np.einsum('xi,yi->yx', db[:, self.pscsfcv_b_i, self.no + self.pscsfcv_b_a], self.xycv_b))

    def osc_str(self, dipole_ao=None):
        """Length-form oscillator strengths (os_sTDA.py:1388-1418); ``dipole_ao`` defaults to
        ``int1e_r`` at the origin, the reference's call."""
        if dipole_ao is None:
            dipole_ao = self._qc_mol().intor_symmetric("int1e_r", comp=3)
        tdip = self._transition(dipole_ao)
        return 2. / 3. * np.einsum('s,sx,sx->s', self.e[:tdip.shape[0]], tdip, tdip)

    def rot_str(self, dip_ele_ao=None, dip_meg_ao=None):
        """Rotatory strengths in cgs units (os_sTDA.py:1420-1468)."""
        if dip_ele_ao is None or dip_meg_ao is None:
            mol = self._qc_mol()
            dip_ele_ao = mol.intor('int1e_ipovlp', comp=3, hermi=2)
            dip_meg_ao = mol.intor('int1e_cg_irxp', comp=3, hermi=2)
        ele = -self._transition(dip_ele_ao)
        meg = 0.5 * self._transition(dip_meg_ao)
        return np.einsum('s,sx,sx->s', 1. / self.e[:ele.shape[0]], ele, meg) / CGS2AU

    def deltaS2(self):
        """Delta<S^2> (os_sTDA.py:1335-1386): the three-term formula on the aligned CV lists
        when spin-adapted, the spin-orbital overlap formula otherwise."""
        if self.spinadapt:
            return (np.einsum('ij,ij->i', self.xycv_a, self.xycv_a) + np.einsum('ij,ij->i', self.xycv_b, self.xycv_b)
                    - 2 * np.einsum('ij,ij->i', self.xycv_a, self.xycv_b))
        nc, no, nv = self.nc, self.no, self.nv
        n = self.v.shape[1]
        coa, cva, cob, cvb = self._orbital_blocks()
        s = self.mf.get_ovlp()
        za = np.zeros((n, nc + no, nv))           # alpha amplitudes [c|o] x v
        zb = np.zeros((n, nc, no + nv))           # beta amplitudes c x [o|v]
        za[:, self.pscsfcv_a_i, self.pscsfcv_a_a] = self.xycv_a
        za[:, nc + self.pscsfov_a_i, self.pscsfov_a_a] = self.xyov_a
        zb[:, self.pscsfco_b_i, self.pscsfco_b_a] = self.xyco_b
        zb[:, self.pscsfcv_b_i, no + self.pscsfcv_b_a] = self.xycv_b
        oo = coa.T @ s @ cob                      # <i_a|j_b>
        va_ob = cva.T @ s @ cob
        vb_oa = cvb.T @ s @ coa
        vv = cva.T @ s @ cvb
        # the sixteen block terms of the reference, summed over whole-spin amplitude matrices
        m_a = oo @ oo.T                           # alpha occupied, projected on beta occupied
        m_b = oo.T @ oo
        return (np.einsum('nia,nja,ij->n', za, za, m_a) - np.einsum('nia,nib,ab->n', za, za, va_ob @ va_ob.T)
                + np.einsum('nia,nja,ij->n', zb, zb, m_b) - np.einsum('nia,nib,ab->n', zb, zb, vb_oa @ vb_oa.T)
                - 2 * np.einsum('nia,njb,ij,ab->n', za, zb, oo, vv))
