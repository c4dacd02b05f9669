"""State-to-state transition moments of spin-flip roots on the device (``xt_tdm``).

The roots of a spin-flip eigenproblem are the target ground state and its excited
states alike, so intensities need the moment *between roots*.  The reference evaluates 16
trace terms per ordered pair and Cartesian component (``XSF_TDA.calculate_TDM_R`` /
``calculate_TDM_U``, XSF_TDA.py:435-592; ``XSF_TDA_GPU.osc_str``, XSF_TDA_GPU.py:936-1116);
the terms are bilinear in the two states, so ``xt_tdm`` applies the operator's image once
per state and takes one Gram product (``include/xtddft_amd.h``).  This module is the thin
host side shared by ``XSF_TDA``, ``SF_TDA_down`` and ``SF_TDA_up``.

The spin-conserving roots of ``XTDA`` (X-TDA / U-TDA) go through ``xt_tdm_sc`` in the same
way (``transition_moments_sc``): ``X_TDA.calculate_TDM`` (xtddft/XTDA.py:1354-1400) over
``TDM_S`` / ``TDM_GSS`` (x2c_hamiltonian/driver/tdm.py:6-126), reference state included.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi


def transition_moments(op_ao, c_occ, c_vir, vecs, nc, no, nv, sa=0, si=0.0, layout="blocks",
                       vects=None, device=0):
    """(ncomp, nstates, nstates) moments <i|op_x|j> of the states in the rows of ``vecs``.

    ``op_ao`` (ncomp, nao, nao) symmetric; ``c_occ`` (nao, nc+no) / ``c_vir`` (nao, no+nv) the
    occupied / virtual coefficients of the amplitude matrix; ``layout`` 'blocks' (the
    reference's cv|co|ov|oo rows, OO compressed when ``vects`` is given) or 'ov' (occ x vir
    row-major); ``sa`` / ``si`` select the spin-adapted factors (XSF_TDA.py:496-507)."""
    import torch
    op_ao = np.ascontiguousarray(op_ao, dtype=np.float64)
    if op_ao.ndim == 2:
        op_ao = op_ao[None]
    c_occ = np.ascontiguousarray(c_occ, dtype=np.float64)
    c_vir = np.ascontiguousarray(c_vir, dtype=np.float64)
    vecs = np.ascontiguousarray(vecs, dtype=np.float64)
    nao = c_occ.shape[0]
    if op_ao.shape[1:] != (nao, nao):
        raise ValueError(f"operator has shape {op_ao.shape}, expected (ncomp, {nao}, {nao})")
    if c_occ.shape != (nao, nc + no) or c_vir.shape != (nao, no + nv):
        raise ValueError("coefficient blocks do not match (nao, nc+no) / (nao, no+nv)")
    compressed = vects is not None
    dim = (nc + no) * (no + nv) - (1 if compressed else 0)
    if vecs.ndim != 2 or vecs.shape[1] != dim:
        raise ValueError(f"state vectors have shape {vecs.shape}, expected (nstates, {dim})")
    ncomp, nstates = op_ao.shape[0], vecs.shape[0]
    if compressed:
        vects = np.ascontiguousarray(vects, dtype=np.float64)
        if vects.shape != (no * no, no * no - 1):
            raise ValueError(f"vects has shape {vects.shape}, expected ({no * no}, {no * no - 1})")
    d = _capi.XtTdmDesc(nao=nao, nc=nc, no=no, nv=nv, ncomp=ncomp, nstates=nstates, sa=int(sa),
                        si=float(si), layout=_capi.TDM_LAYOUT[layout], oo_compressed=int(compressed))
    out = np.empty((ncomp, nstates, nstates))
    L = _capi.lib()
    dev = torch.device(f"cuda:{device}")
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(L.xt_tdm(ctypes.byref(d), op_ao.ctypes.data, c_occ.ctypes.data, c_vir.ctypes.data,
                             vecs.ctypes.data, vects.ctypes.data if compressed and vects.size else None,
                             out.ctypes.data, _capi.XT_PTR_HOST, ctypes.c_void_p(st)), "xt_tdm")
    return out


def transition_moments_sc(op_ao, c_occ_a, c_vir_a, c_occ_b, c_vir_b, vecs, spin_adapted=False, no=0, si=0.0,
                          ground=True, device=0):
    """(ncomp, n, n) moments between the spin-conserving states in the rows of ``vecs``
    (``xt_tdm_sc``), n = nstates + 1 with the reference state as row / column 0 when ``ground``.

    ``vecs`` (nstates, dim) in PySCF order [za (nocc_a x nvir_a) | zb (nocc_b x nvir_b)];
    ``spin_adapted`` adds the X-TDA correction of a ROKS reference with ``no`` open shells and
    spin ``si`` (TDM_S, x2c_hamiltonian/driver/tdm.py:61-126).  In the phase of
    ``utils.so2st``, cv1 = (cva - cvb)/sqrt(2), the couplings of CV(1) with CO(0) and OV(0)
    carry -sqrt((S+1)/(2S)); tdm.py writes + for a CV(1) of the opposite sign."""
    import torch
    op_ao = np.ascontiguousarray(op_ao, dtype=np.float64)
    if op_ao.ndim == 2:
        op_ao = op_ao[None]
    cs = [np.ascontiguousarray(c, dtype=np.float64) for c in (c_occ_a, c_vir_a, c_occ_b, c_vir_b)]
    vecs = np.ascontiguousarray(vecs, dtype=np.float64)
    nao = cs[0].shape[0]
    if op_ao.shape[1:] != (nao, nao):
        raise ValueError(f"operator has shape {op_ao.shape}, expected (ncomp, {nao}, {nao})")
    if any(c.ndim != 2 or c.shape[0] != nao for c in cs):
        raise ValueError("coefficient blocks must be (nao, n) arrays of one nao")
    oa, va, ob, vb = (c.shape[1] for c in cs)
    dim = oa * va + ob * vb
    if vecs.ndim != 2 or vecs.shape[1] != dim:
        raise ValueError(f"state vectors have shape {vecs.shape}, expected (nstates, {dim})")
    ncomp, nstates = op_ao.shape[0], vecs.shape[0]
    d = _capi.XtTdmScDesc(nao=nao, nocc_a=oa, nvir_a=va, nocc_b=ob, nvir_b=vb, ncomp=ncomp, nstates=nstates,
                          spin_adapted=int(bool(spin_adapted)), no=int(no), si=float(si),
                          with_ground=int(bool(ground)))
    n = nstates + int(bool(ground))
    out = np.empty((ncomp, n, n))
    L = _capi.lib()
    dev = torch.device(f"cuda:{device}")
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(L.xt_tdm_sc(ctypes.byref(d), op_ao.ctypes.data, *(c.ctypes.data if c.size else None for c in cs),
                                vecs.ctypes.data, out.ctypes.data, _capi.XT_PTR_HOST, ctypes.c_void_p(st)),
                    "xt_tdm_sc")
    return out


def charge_centre_dipole(mf, mol=None):
    """``int1e_r`` (3, nao, nao) with the origin at the centre of nuclear charge
    (XSF_TDA.py:482-487), from a Mole that has integrals (``xtddft_amd.qc``)."""
    for m in (mol, getattr(mf, "mol", None), mf.extra.get("qc_mol")):
        if m is not None and hasattr(m, "intor_symmetric"):
            charges = np.asarray(m.atom_charges(), dtype=np.float64)
            origin = np.einsum('z,zr->r', charges, m.atom_coords()) / charges.sum()
            return m.intor_symmetric("int1e_r", comp=3, origin=tuple(origin))
    raise ValueError("transition dipoles need AO dipole integrals: pass op_ao or a Mole with intor")


def osc_matrix(e, tdm):
    """(2/3) |e_i - e_j| sum_x T_x[i,j]^2 (XSF_TDA.py:591, XSF_TDA_GPU.osc_str)."""
    e = np.asarray(e, dtype=np.float64)
    return 2.0 / 3.0 * np.abs(e[:, None] - e[None, :]) * np.einsum('xij,xij->ij', tdm, tdm)


def tdm_tables_sc(e, tdm):
    """The two tables X_TDA.calculate_TDM prints (XTDA.py:1371-1400) from the excitation
    energies ``e`` (n) and the moments ``tdm`` (3, n+1, n+1) with the reference state as row /
    column 0: a title and one line per excited state, a blank line, then a title, a header and
    one line per ordered pair of excited states.  As in the reference the last column of a
    pair line is signed, f(L<-R) = (2/3)(e_L - e_R) sum_x T_x^2."""
    e = np.asarray(e, dtype=np.float64)
    n = e.size
    t2 = np.einsum('xij,xij->ij', tdm, tdm)
    lines = ["Ground state to Excited state transition dipole moments(a.u.)"]
    for i in range(n):
        t = tdm[:, i + 1, 0]
        lines.append(f' {i + 1:2d}     |GS⟩    {t[0]:>8.4f} {t[1]:>8.4f} {t[2]:>8.4f}  '
                     f'{2 / 3 * e[i] * t2[i + 1, 0]:>8.4f} ')
    lines += ["", "Excited state to Excited state transition dipole moments(a.u.)",
              "StateL StateR      X        Y        Z      f(L<-R)"]
    for i in range(n):
        for j in range(n):
            t = tdm[:, i + 1, j + 1]
            lines.append(f' {i + 1:2d}     {j + 1:2d}    {t[0]:>8.4f} {t[1]:>8.4f} {t[2]:>8.4f}  '
                         f'{2 / 3 * (e[i] - e[j]) * t2[i + 1, j + 1]:>8.4f} ')
    return lines


def tdm_table(tdm, osc):
    """The reference's printed table (XSF_TDA.py:493-494, 592): a title, a header and one
    line per ordered pair of states."""
    lines = ["Excited state to Excited state transition dipole moments(Au)",
             "State State    X     Y     Z     OSC."]
    n = osc.shape[0]
    for i in range(n):
        for j in range(n):
            t = tdm[:, i, j]
            lines.append(f'{i + 1:2d} {j + 1:2d} {t[0]:>8.4f} {t[1]:>8.4f} {t[2]:>8.4f}  {osc[i, j]:>8.4f} ')
    return lines
