"""Analytic nuclear gradients of U-TDA (spin-conserving TDA) states on a UHF or UKS reference: the
reference's ``xtddft/grad_jp/grad/utdhf.py`` with Y = 0, extended to LDA / GGA functionals (pure
or global hybrid) as PySCF's ``grad.tduks`` is,

    td = XTDA(mol, mf); td.kernel()
    g = td.nuc_grad_method()                   # UTDAGradients
    g.state = 2                                # 1-based
    de = g.kernel()                            # (natm, 3) Ha / Bohr, d(E_SCF + omega_state)/dR

With X_s (nvir_s, nocc_s) the amplitudes of one root, |X_a|^2 + |X_b|^2 = 1, Xt_s = C_v X_s C_o^T,
X_S = (Xt + Xt^T) / 2 and X_A = (Xt - Xt^T) / 2 per spin, the functional that is differentiated is

    omega = sum_s tr(X_s^T F_vv,s X_s) - tr(X_s F_oo,s X_s^T) + X_S,tot : J[X_S,tot]
            - hyb sum_s (X_S,s : K[X_S,s] + X_A,s : K[X_A,s]) + sum_g rho1(g) . wv[X_S](g)

(hyb = 1 and no XC term on Hartree-Fock); rho1 and wv = w fxc rho1 are what ``xt_xc_resp`` returns for
the pair (X_S,a, X_S,b).  The coupling applied to X is G_s = J[X_S,tot] - hyb K[Xt_s] + V^resp_s[X_S]
(d omega = 2 dXt_s : G_s), and the Lagrangian follows the working spin-flip ``grad.grad_elec`` with
-hyb K[X] replaced by G_s and both blocks of T in both spins:

    T_s        = C_v X X^T C_v^T - C_o X^T X C_o^T
    veff0doo_s = J[T_a + T_b] - hyb K[T_s] + the potential of wv[T] + wv2,   wv2 = w d(rho1^T fxc rho1)/d rho0
    rhs_s      = 2 (C_v^T veff0doo_s C_o + G_vv^T X - X G_oo^T)              (Z-vector, ``qc.grad.solve_zvector``)
    W_oo = F_oo + C_o^T (veff0doo + veff[Z^S]) C_o - X^T X F_oo + X^T G_vo,   W_vv = X X^T F_vv + X G_vo^T,
    W_vo = Z F_oo + 2 X G_oo^T.

wv2 is the third functional derivative contracted twice with rho1 (PySCF's ``k1ao``): two directional
derivatives of the energy density and one backward pass (``qc.xc.kernel_grad_torch``), no
third-derivative tensor.  The two-electron derivative term is ONE ``xt_grad_jk2`` call
(``qc.grad.grad_jk_lists``) with, for D = D0 + T + Z^S and TZ = T + Z^S per spin,

    Coulomb list:   (+1; D_tot, D_tot), (-1; TZ_tot, TZ_tot), (+2; X_S,tot, X_S,tot)
    exchange list:  per spin, scaled by hyb: (-1; D_s, D_s), (+1; TZ_s, TZ_s) and the X_S / X_A exchange
                    4 hyb (X_S[a,c] X_S[b,d] + X_A[a,c] X_A[b,d]) = 2 hyb (Xt[a,c] Xt[b,d] + Xt^T[a,c] Xt^T[b,d])

in the weights of ``qc.grad.jk_terms``: three Coulomb and eight exchange pairs on a hybrid, none of
the latter on a pure functional.  The XC nuclear-derivative term (``qc.grad.grad_xc_pairs``) is
G_xc[w vxc[rho0]; D0 + T + Z^S] + G_xc[wv[T + Z^S] + wv2; D0] + G_xc[2 wv[X_S]; X_S] on a grid held fixed
in space.

Refused with NotImplementedError: an ROKS / ROHF mean field (X-TDA: the reference's ``xtdhf.py``),
``basis='tensor'``, a Kohn-Sham mean field on the host, and everything ``qc.grad.check_gradient_mf`` /
``check_ks_gradient_mf`` refuse (meta-GGA, range separation, VV10, density fitting, X2C).

Range-separated hybrids come in through ``td.Gradients(state=1)``, which constructs
``UTDAGradients(td, allow_rsh=True)``: -hyb K above becomes -(hyb K + (alpha - hyb) K_LR) everywhere, and the
exchange list goes once through ``xt_grad_jk2`` weighted by hyb and once through ``xt_grad_jk2_lr`` weighted
by alpha - hyb (``qc.grad.grad_2e``: ``grad_jk_rsh``).  ``nuc_grad_method()`` keeps refusing them.

The driver object, the XC hook and the resolution of the reference are shared with the spin-flip gradients:
``UTDAGradients``, ``KSTerms`` and ``_scf_of`` build on ``grad_common``.
"""
from __future__ import annotations

import time

import numpy as np

from . import grad_common as _c
from .qc import grad as _g


def _scf_of(td, allow_rsh=False):
    """(the SCF object behind ``td.mf``, whether it is a Kohn-Sham reference) after every refusal.
    ``allow_rsh``: the caller came through ``.Gradients()``, which takes range-separated hybrids."""
    mf = td.mf
    if getattr(td, "X", False) or getattr(mf, "is_rohf", False):
        raise NotImplementedError("X-TDA gradients on an ROKS / ROHF reference (the reference's grad_jp/grad/xtdhf.py) "
                                  "are not built: the restricted open-shell determinant is not variational in the "
                                  "rotations the U-TDA formula assumes; use a UHF / UKS reference")
    if td.basis == 'tensor':
        raise NotImplementedError("U-TDA gradients need basis='orbital': the tensor-basis solver is not built")
    scf = _c.scf_behind(mf)
    if scf is None:
        raise ValueError("the gradient needs the SCF object the mean field came from (qc UHF / UKS .to_meanfield()), "
                         "still alive")
    return scf, _c.check_reference(scf, "U-TDA", allow_rsh)


def utda_amplitudes(td, state_idx):
    """(X_a (nvir_a, nocc_a), X_b (nvir_b, nocc_b)) of root ``state_idx`` (0-based), normalised to
    |X_a|^2 + |X_b|^2 = 1: ``td.v`` holds [CV(aa) | OV(aa) | CO(bb) | CV(bb)] (``XTDA._split_blocks``); the
    alpha part is already (occupied, virtual) row-major, the beta part goes back through ``td.order``."""
    v = np.asarray(td.v)[:, state_idx]
    nc, no, nv = td.nc, td.no, td.nv
    na = (nc + no) * nv
    xa = v[:na].reshape(nc + no, nv)
    b = np.zeros(nc * (no + nv))
    b[np.asarray(td.order)[na:] - na] = v[na:]
    xb = b.reshape(nc, no + nv)
    nrm = np.linalg.norm(v)
    return xa.T / nrm, xb.T / nrm


class KSTerms(_c.KSTerms):
    """The XC terms of ``grad_elec`` on a UKS reference (LDA / GGA): ``grad_common.KSTerms`` in the order
    alpha, beta, with the coupling of the reference's own kernel and its third-derivative weights wv2
    (``qc.xc.kernel_grad_torch``); the extra pair is G_xc[2 wv[X_S]; X_S]."""

    def coupling(self, x_s):
        """V^resp (2, nao, nao) of the symmetric transition densities X_S; keeps wv1 = wv[X_S] and
        wv2 = w d(rho1^T fxc rho1) / d rho0 for ``vxc_resp_t`` and ``grad``."""
        import torch
        from .qc import xc as _xc
        eng, nk = self.eng, self.nk
        out = self._timed(eng.fxc_response, x_s, want=("v", "wv", "rho1"))
        t0 = time.perf_counter()
        with torch.cuda.device(eng.dev):
            _, dq = _xc.kernel_grad_torch(self.scf.xc, self.rho0()[:, :nk], out["rho1"][:, :nk])
            wv2 = self._kernel_weights(dq)
        torch.cuda.synchronize(eng.dev)
        self.tm["kernel_grad_s"] = time.perf_counter() - t0
        self.x_s, self.wv1, self.wv2 = np.asarray(x_s), out["wv"], wv2
        return out["v"]

    def _rows_done(self, seconds):
        self.tm["xc_rows_s"] = seconds

    def extra_pairs(self):
        return [(2.0 * self.wv1, self.x_s)]


def jk_lists(d, tz, xt, hyb):
    """(Coulomb list [(wj, P, Q)], exchange list [(wk, P, Q)]) of the two-electron derivative term:
    d, tz, xt (2, nao, nao) = D0 + T + Z^S, T + Z^S and Xt = C_v X C_o^T per spin (module docstring)."""
    dt, tzt = d[0] + d[1], tz[0] + tz[1]
    xst = sum((m + m.T) * 0.5 for m in xt)

    def j(c, m):
        wj, _, p, q = _g.jk_terms(c, 0, m, m)
        return (wj, p, q)

    def k(c, m):
        _, wk, p, q = _g.jk_terms(0, c, m, m)
        return (wk, p, q)
    jl = [j(1, dt), j(-1, tzt), j(2, xst)]
    kl = []
    if hyb != 0:
        for s in range(2):
            kl += [k(-hyb, d[s]), k(hyb, tz[s]), (2.0 * hyb, xt[s], xt[s]), (2.0 * hyb, xt[s].T, xt[s].T)]
    return jl, kl


def grad_elec(scf, x, device, cphf_conv_tol=1e-10, cphf_max_cycle=500, timings=None, hyb=1.0, xc=None, rsh=None,
              root=None):
    """Electronic part of the gradient of E_SCF + omega, (natm, 3).  ``x`` = (X_a, X_b), each
    (nvir_s, nocc_s); ``hyb``: the fraction of exact exchange (1 for Hartree-Fock); ``xc``: the XC terms
    of a UKS reference (``KSTerms``), None for Hartree-Fock.  The two-electron derivative term is one
    ``xt_grad_jk2`` call.
    ``rsh``: (omega, alpha) of a range-separated hybrid: every K below is hyb K + (alpha - hyb) K_LR
    (``qc.grad.exchange_jk`` here, ``qc.grad.ks_response`` in the Z-vector) and the exchange list goes once per
    operator (``qc.grad.grad_2e``: ``grad_jk_rsh``); ``root``: the TDA root (Ha) of these amplitudes, checked
    against the omega of the coupling formed here (``grad.check_root``)."""
    tm = {} if timings is None else timings
    mol = scf.mol
    C = [np.asarray(scf.mo_coeff[s]) for s in range(2)]
    occ = [np.asarray(scf.mo_occ[s]) > 0 for s in range(2)]
    o = [C[s][:, occ[s]] for s in range(2)]
    v = [C[s][:, ~occ[s]] for s in range(2)]
    no = [o[s].shape[1] for s in range(2)]
    fock_ao = scf.get_hcore()[None] + np.asarray(scf._veff)       # a UKS _veff holds V_xc
    F = [C[s].T @ fock_ao[s] @ C[s] for s in range(2)]
    x = [np.asarray(x[s], dtype=np.float64) for s in range(2)]
    for s in range(2):
        if x[s].shape != (v[s].shape[1], no[s]):
            raise ValueError(f"amplitude shape {x[s].shape}, expected {(v[s].shape[1], no[s])}")

    get_jk = _g.exchange_jk(scf, hyb, rsh)

    too = [-x[s].T @ x[s] for s in range(2)]
    tvv = [x[s] @ x[s].T for s in range(2)]
    dmt = np.asarray([v[s] @ tvv[s] @ v[s].T + o[s] @ too[s] @ o[s].T for s in range(2)])
    dmt = (dmt + dmt.transpose(0, 2, 1)) * 0.5
    xt = np.asarray([v[s] @ x[s] @ o[s].T for s in range(2)])
    xs = (xt + xt.transpose(0, 2, 1)) * 0.5
    vj, vk = get_jk((dmt[0], dmt[1], xt[0], xt[1]))               # vk carries hyb from here on
    jx = vj[2] + vj[3]                                            # J[Xt_tot] = J[X_S,tot]
    jx = (jx + jx.T) * 0.5
    G = [jx - vk[2 + s] for s in range(2)]
    veff0doo = [vj[0] + vj[1] - vk[s] for s in range(2)]
    if xc is not None:
        vx = xc.coupling(xs)
        fxt = xc.vxc_resp_t(dmt)
        G = [G[s] + vx[s] for s in range(2)]
        veff0doo = [veff0doo[s] + fxt[s] for s in range(2)]
    gmo = [C[s].T @ G[s] @ C[s] for s in range(2)]
    if root is not None:         # omega = sum_s tr(X^T F_vv X) - tr(X F_oo X^T) + Xt_s : G_s
        from .grad import check_root
        check_root("U-TDA gradient", float(sum(np.sum(x[s] * (
            F[s][no[s]:, no[s]:] @ x[s] - x[s] @ F[s][:no[s], :no[s]] + gmo[s][no[s]:, :no[s]])) for s in range(2))),
            float(root))
    # right-hand side of the Z-vector equations
    wvo = [2.0 * (v[s].T @ veff0doo[s] @ o[s] + gmo[s][no[s]:, no[s]:].T @ x[s] - x[s] @ gmo[s][:no[s], :no[s]].T)
           for s in range(2)]
    t0 = time.perf_counter()
    za, zb, res, ncyc = _g.solve_zvector(scf, wvo[0], wvo[1], cphf_conv_tol, cphf_max_cycle,
                                         vresp=None if xc is None else xc.vresp)
    tm["zvector_s"] = time.perf_counter() - t0
    tm["zvector_cycles"], tm["zvector_residual"] = ncyc, float(res)
    z = [za, zb]
    z1ao = np.asarray([v[s] @ z[s] @ o[s].T for s in range(2)])
    zs = (z1ao + z1ao.transpose(0, 2, 1)) * 0.5
    veff = _g.hf_response(scf)(zs) if xc is None else xc.vresp(zs)      # J - hyb K (+ V^resp) of Z^S
    # energy-weighted density W
    im0 = 0.0
    for s in range(2):
        n = no[s]
        w = np.zeros_like(F[s])
        w[:n, :n] = (F[s][:n, :n] + o[s].T @ (veff0doo[s] + veff[s]) @ o[s] + too[s] @ F[s][:n, :n]
                     + x[s].T @ gmo[s][n:, :n])
        w[n:, n:] = tvv[s] @ F[s][n:, n:].T + x[s] @ gmo[s][n:, :n].T
        w[n:, :n] = z[s] @ F[s][:n, :n].T + 2.0 * x[s] @ gmo[s][:n, :n].T
        im0 = im0 + C[s] @ w @ C[s].T
    d0 = np.asarray([o[s] @ o[s].T for s in range(2)])
    tz = zs + dmt
    t0 = time.perf_counter()
    de = _g.contract_1e(mol, _g.hcore_generator(mol), _g.get_ovlp(mol), (d0 + tz).sum(axis=0), im0)
    tm["one_electron_s"] = time.perf_counter() - t0
    # range-separated: the pairs of full exchange, weighted per operator, two calls
    lists = jk_lists(d0 + tz, tz, xt, hyb if rsh is None else 1.0)
    de += _g.grad_2e(mol, device, tm, hyb, rsh, lists=lists)
    if xc is not None:
        de += xc.grad(d0, tz)
    return de


class UTDAGradients(_c.TDAGradients):
    """``XTDA(mol, mf).nuc_grad_method()`` on a UHF or UKS (LDA / GGA, pure or global hybrid, on a
    device) reference, with the attributes of ``grad.SFGradients`` (``grad_common.TDAGradients``).
    ``timings`` of the last gradient: ``one_electron_s``, ``grad_jk_s`` and ``buckets``, ``zvector_s`` /
    ``zvector_cycles`` / ``zvector_residual`` and, on a UKS reference, ``xc_response_s`` /
    ``xc_response_calls`` (every V^resp / wv evaluation, the Z-vector's included), ``kernel_grad_s`` (the
    third-derivative weights), ``xc_rows_s`` and ``grad_xc_s``."""

    _name, _not_run = "XTDA", ValueError

    def __init__(self, td, *, allow_rsh=False):
        super().__init__(td, *_scf_of(td, allow_rsh))

    def _davidson(self):
        return self.base.use_Davidson

    def _amplitudes(self):
        return utda_amplitudes(self.base, self.state - 1)

    def _ks_terms(self):
        return KSTerms(self._scf, self.timings, self.xc_chunk)

    def _grad_elec(self, x, device, **kw):
        return grad_elec(self._scf, x, device, self.cphf_conv_tol, self.cphf_max_cycle, self.timings, **kw)
