"""State-to-state transition moments of spin-flip roots on the device (``xt_tdm``).

The roots of a spin-flip eigenproblem are the target ground state and its excited
states alike, so intensities need the moment *between roots*.  The reference evaluates 16
trace terms per ordered pair and Cartesian component (``XSF_TDA.calculate_TDM_R`` /
``calculate_TDM_U``, XSF_TDA.py:435-592; ``XSF_TDA_GPU.osc_str``, XSF_TDA_GPU.py:936-1116);
the terms are bilinear in the two states, so ``xt_tdm`` applies the operator's image once
per state and takes one Gram product (``include/xtddft_amd.h``).  This module is the thin
host side shared by ``XSF_TDA``, ``SF_TDA_down`` and ``SF_TDA_up``.
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
