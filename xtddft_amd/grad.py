"""Analytic nuclear gradients of spin-flip TDA (CIS) states on a UHF or UKS reference: the reference's
USF-CIS gradient (``xtddft/grad_jp/grad/usfcis.py``) with its API,

    g = SF_TDA_down(mf).nuc_grad_method()      # or SF_TDA_up(mf)
    g.state = 2                                # 1-based, as the reference
    de = g.kernel()                            # (natm, 3) Ha / Bohr

``grad_elec`` follows usfcis.py:16-256 in content: the relaxed-density pieces T_alpha, T_beta and
the symmetric / antisymmetric parts of the transition density (85-95), the Lagrangian right-hand
side Q / w (104-126), the Z-vector (127-150, ``qc.grad.solve_zvector``: J / K on the device), the
energy-weighted density W (``im0``, 158-183) and the final contraction (193-253).  Its
``td_grad.get_jk`` / ``get_k`` derivative-integral terms -- ground state, T + Z and X_S / X_A --
are the terms of **one** ``xt_grad_jk`` call (``qc.grad.grad_jk_device``); with D = D0 + (T + Z^S)
the cross terms of ground state and T + Z are D x D - (T + Z^S) x (T + Z^S), which keeps the
call at the kernel's eight density pairs.

Spin-flip-up is the same derivation with alpha and beta exchanged (J / K of a Hartree-Fock
reference do not tell the spins apart): the driver hands the spin-reversed orbitals to the
same function.

On a UKS reference (LDA / GGA, pure or global hybrid, after ``to_device()``) the same function gives
the collinear (``method = 2``) spin-flip TDA gradient, the content of the reference's
``grad_hb/tduks_sfu.py:184-369`` with f1vo = k1ao = 0: every K carries ``hyb``, f^xc[T] joins
``veff0doo``, the Z-vector operator is the UKS response (``qc.grad.ks_response``: J - hyb K +
V^resp through ``xt_xc_resp``) and the XC nuclear-derivative term is
G_xc[w vxc[rho0]; D0 + T + Z^S] + G_xc[wv[T + Z^S]; D0] (``qc.grad.grad_xc_pairs``), on a grid held
fixed in space.

The multicollinear kernel (``method = 1``) keeps f1vo and k1ao: with
omega_xc = sum_g w 2 rho1^T fxc_sf(rho0) rho1, rho1 of the symmetrised transition density X_S, f1vo is
the potential V_sf of wv1 = 2 w fxc_sf rho1 (``xt_xc_resp_sf``), which stands next to hyb K[X] in the
coupling matrix, and k1ao the potential of wv2 = w d(2 rho1^T fxc_sf rho1) / d rho0
(``mcol.sf_mc_kernel_grad``: one backward pass of that scalar, no third-derivative tensor), which
joins f^xc[T] (``xt_xc_rows``); the XC nuclear-derivative term gains G_xc[wv2; D0] + 2 G_xc[wv1; X_S].
Its entry is ``SFU_gradient`` / ``SFD_gradient``, the reference's own names; ``nuc_grad_method()`` keeps
refusing method = 1 and names them.

Refused with NotImplementedError: on a UHF reference method != 0; on a UKS reference method = 0
(the ALDA0 kernel's density derivative), a mean field on the host, and everything ``qc.grad.check_ks_gradient_mf`` refuses
(meta-GGA, range-separated, VV10, ROKS); density fitting, X2C and an ROHF reference on either.

Range-separated hybrids (CAM-B3LYP, wB97X-D) come in through ``td.Gradients(state=1)``,
which builds the same objects with ``allow_rsh=True``: every K above is hyb K + (alpha - hyb) K_LR
(``qc.grad.exchange_jk``, the ``get_jk`` of ``grad_elec``, and ``qc.grad.ks_response``), and the kernel pairs go
as two lists through ``xt_grad_jk2`` and ``xt_grad_jk2_lr`` (``qc.grad.grad_2e``: ``grad_jk_rsh``).
``nuc_grad_method()``, ``SFU_gradient(td)`` and ``SFD_gradient(td)`` with default arguments keep refusing them.

The driver object, the XC hook and the resolution of the reference are shared with the U-TDA gradients:
``SFGradients``, ``KSTerms`` and ``_scf_of`` build on ``grad_common``.
"""
from __future__ import annotations

import time

import numpy as np

from . import grad_common as _c
from .qc import grad as _g


def _scf_of(td, multicollinear=False, allow_rsh=False):
    """(the SCF object behind ``td.mf``, whether it is a Kohn-Sham reference) after every refusal.
    ``multicollinear``: the caller is ``SFU_gradient`` / ``SFD_gradient``, which take method = 1;
    ``allow_rsh``: the caller came through ``.Gradients()``, which takes range-separated hybrids."""
    mf = td.mf
    if getattr(mf, "is_rohf", False):
        raise NotImplementedError("spin-flip gradients need a UHF / UKS reference (the reference's "
                                  "usfcis-rohf.py is not a working code path; tdroks_sfu.py is not built)")
    scf = _c.scf_behind(mf)
    if scf is None:
        if str(getattr(mf, "xctype", "HF")) != "HF":
            raise NotImplementedError(f"spin-flip gradients for xc = {mf.xc!r} need the qc UKS object the mean "
                                      "field came from (UKS.to_meanfield()), still alive")
        raise ValueError("the gradient needs the SCF object the mean field came from (qc UHF.to_meanfield()), "
                         "still alive")
    if _c.is_hartree_fock(scf) and td.method != 0:
        raise NotImplementedError("spin-flip gradients on a Hartree-Fock reference are built for method = 0 only")
    if not _c.check_reference(scf, "spin-flip", allow_rsh):
        return scf, False
    if td.method == 0:
        raise NotImplementedError("spin-flip gradients with the ALDA0 kernel (method = 0) on a functional: the "
                                  "density derivative of the ALDA0 kernel is not built (method = 2 is)")
    if td.method == 1 and not multicollinear:
        raise NotImplementedError("spin-flip gradients with the multicollinear kernel (method = 1) come from "
                                  "xtddft_amd.grad.SFU_gradient(td) / SFD_gradient(td), the reference's own entry "
                                  "(grad_hb/tduks_sfu.py); nuc_grad_method() gives the collinear kernel, method = 2")
    return scf, True


def sf_amplitude(td, state_idx):
    """x (nvir_f, nocc_i) of root ``state_idx`` (0-based), normalised: flipped-to virtuals by
    flipped-from occupieds (usfcis.py:61-73 for spin-flip-down; spin-flip-up is stored (o, v))."""
    v = np.asarray(td.v)[:, state_idx]
    nc, no, nv = td.nc, td.no, td.nv
    if td.isf == -1:
        d1, d2, d3 = nc * nv, nc * nv + nc * no, nc * nv + nc * no + no * nv
        x = np.zeros((nc + no, no + nv))
        x[:nc, :no] = v[d1:d2].reshape(nc, no)
        x[:nc, no:] = v[:d1].reshape(nc, nv)
        x[nc:, :no] = v[d3:].reshape(no, no)
        x[nc:, no:] = v[d2:d3].reshape(no, nv)
    else:
        x = v.reshape(nc, nv)
    return x.T / np.linalg.norm(x)


class KSTerms(_c.KSTerms):
    """The XC hook of ``grad_elec`` for a UKS reference (LDA / GGA): ``grad_common.KSTerms`` in the labels of
    ``grad_elec``, "a" = flipped-from, "b" = flipped-to (``s``), with the coupling of the multicollinear kernel
    (``sf_coupling``); the collinear kernel has none, and neither wv2 nor an extra pair."""

    def __init__(self, scf, s, timings, xc_chunk=None, mc=None):
        """``mc``: None for the collinear kernel; for the multicollinear one a dict
        with ``mf`` (the mean field of the TDA object) and ``samples`` (the sample count its roots were
        computed with)."""
        self.s, self.mc = s, mc
        super().__init__(scf, timings, xc_chunk)   # multicollinear: wv1 (4, G), wv2 (2, 4, G) alpha, beta

    def _order(self, pair):
        return np.asarray([pair[self.s[0]], pair[self.s[1]]])     # s is its own inverse

    def sf_coupling(self, x_s):
        """V_sf (nao, nao), the potential of wv1 = 2 w fxc_sf rho1[X_S], which stands next to hyb K[X] in
        the coupling matrix; None with the collinear kernel.  Keeps wv1 and wv2 = w d(2 rho1^T fxc_sf
        rho1) / d rho0 (``mcol.sf_mc_kernel_grad``) for ``vxc_resp_t`` and ``grad``."""
        if self.mc is None:
            return None
        import torch
        from .mcol import sf_mc_kernel, sf_mc_kernel_grad
        eng, mf, ns = self.eng, self.mc["mf"], self.mc["samples"]
        kern = sf_mc_kernel(mf, ns, device=eng.dev.index)
        t0 = time.perf_counter()
        out = eng.fxc_sf_response(x_s, kern, want=("v", "wv", "rho1"))
        torch.cuda.synchronize(eng.dev)
        self.tm["xc_sf_response_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, dq = sf_mc_kernel_grad(mf, out["rho1"][:self.nk], ns, device=eng.dev.index, rho=self.rho0())
        wv2 = self._kernel_weights(dq)
        torch.cuda.synchronize(eng.dev)
        self.tm["mc_kernel_grad_s"] = time.perf_counter() - t0
        self.x_s, self.wv1, self.wv2 = np.asarray(x_s), out["wv"], wv2
        return out["v"]

    def vxc_resp_t(self, dm):
        """f^xc[T], and with the multicollinear kernel V^k, the potential of wv2, from the same row pass."""
        return self.vxc_resp(dm) if self.mc is None else super().vxc_resp_t(dm)

    def _rows_done(self, seconds):
        self.tm["xc_sf_response_s"] += seconds

    def extra_pairs(self):
        """2 G_xc[wv1; X_S] with the multicollinear kernel: a one-channel term, run as a two-spin pair whose
        second channel is zero."""
        if self.mc is None:
            return []
        import torch
        h1 = torch.zeros_like(self.wv2)
        h1[0] = 2.0 * self.wv1
        return [(h1, np.asarray([self.x_s, np.zeros_like(self.x_s)]))]


OMEGA_TOL = 1e-9         # Ha: how closely the omega of the gradient's own coupling must reproduce the TDA root


def check_root(what, omega, root):
    """The excitation energy the gradient's coupling gives for the amplitudes against the root of the TDA
    solve: they differ when the operator's exchange and the gradient's do (a missing long-range term)."""
    if abs(omega - root) > OMEGA_TOL:
        raise AssertionError(f"{what}: the coupling of the gradient gives omega = {omega:.12f} Ha for these "
                             f"amplitudes, the TDA root is {root:.12f} Ha (difference {omega - root:.3e} > "
                             f"{OMEGA_TOL:.0e}): the gradient would not be the derivative of that root")


def grad_elec(scf, x_ab, flip, device, cphf_conv_tol=1e-10, cphf_max_cycle=500, timings=None, hyb=1.0, xc=None,
              rsh=None, root=None):
    """Electronic part of the gradient of E_SCF + omega, (natm, 3).  ``x_ab`` (nvir_b, nocc_a) in
    the labels of spin-flip-down; ``flip``: the state is spin-flip-up, and "a" below is beta.
    ``hyb``: the fraction of exact exchange (1 for Hartree-Fock) on every K; ``xc``: the XC terms of a
    UKS reference (``KSTerms``), None for Hartree-Fock, which then runs exactly the UHF formula.
    ``rsh``: (omega, alpha) of a range-separated hybrid, whose exchange is hyb K + (alpha - hyb) K_LR in
    every place K stands below (all of them go through ``get_jk``) and in the kernel lists
    (``qc.grad.grad_jk_rsh``); ``root``: the TDA root (Ha) these amplitudes belong to, checked against the
    omega of the coupling formed here (``check_root``)."""
    tm = {} if timings is None else timings
    mol = scf.mol
    s = (1, 0) if flip else (0, 1)
    mo_coeff = [scf.mo_coeff[s[0]], scf.mo_coeff[s[1]]]
    mo_occ = [scf.mo_occ[s[0]], scf.mo_occ[s[1]]]
    fock_ao = scf.get_hcore()[None] + np.asarray(scf._veff)       # a UKS _veff holds V_xc
    orboa, orbva = mo_coeff[0][:, mo_occ[0] > 0], mo_coeff[0][:, mo_occ[0] == 0]
    orbob, orbvb = mo_coeff[1][:, mo_occ[1] > 0], mo_coeff[1][:, mo_occ[1] == 0]
    nocca, noccb = orboa.shape[1], orbob.shape[1]
    fockamo = mo_coeff[0].T @ fock_ao[s[0]] @ mo_coeff[0]
    fockbmo = mo_coeff[1].T @ fock_ao[s[1]] @ mo_coeff[1]
    if x_ab.shape != (orbvb.shape[1], nocca):
        raise ValueError(f"amplitude shape {x_ab.shape}, expected {(orbvb.shape[1], nocca)}")

    get_jk = _g.exchange_jk(scf, hyb, rsh)

    # T_alpha (occupied-occupied), T_beta (virtual-virtual), X in the AO basis
    ta = -x_ab.T @ x_ab
    tb = x_ab @ x_ab.T
    dmta = orboa @ ta @ orboa.T
    dmtb = orbvb @ tb @ orbvb.T
    dmxab = orbvb @ x_ab @ orboa.T
    dmSx, dmAx = (dmxab + dmxab.T) / 2, (dmxab - dmxab.T) / 2
    vj, vk = get_jk((dmta, dmtb, dmSx, dmAx))                     # vk carries hyb from here on
    kx = vk[2] + vk[3]                                            # K[X_S] + K[X_A]
    vsf = None if xc is None else xc.sf_coupling(dmSx)            # multicollinear kernel: hyb K[X] - V_sf
    if vsf is not None:
        kx = kx - vsf
    vkmo = mo_coeff[1].T @ kx @ mo_coeff[0]                       # beta rows, alpha columns
    if root is not None:         # omega = x . (F_vv x - x F_oo - K[X]_vo)
        check_root("spin-flip gradient", float(np.sum(x_ab * (
            fockbmo[noccb:, noccb:] @ x_ab - x_ab @ fockamo[:nocca, :nocca] - vkmo[noccb:, :nocca]))), float(root))
    veff0dooa = vj[0] + vj[1] - vk[0]
    veff0doob = vj[0] + vj[1] - vk[1]
    if xc is not None:           # f^xc[T] (+ V^k)
        fxt = xc.vxc_resp_t(((dmta + dmta.T) * 0.5, (dmtb + dmtb.T) * 0.5))
        veff0dooa, veff0doob = veff0dooa + fxt[0], veff0doob + fxt[1]
    # right-hand side of the Z-vector equations
    wvoa = 2.0 * (orbva.T @ veff0dooa @ orboa + fockamo[nocca:, :nocca] @ ta.T - vkmo[noccb:, nocca:].T @ x_ab)
    wvob = 2.0 * (orbvb.T @ veff0doob @ orbob - tb @ fockbmo[:noccb, noccb:].T + x_ab @ vkmo[:noccb, :nocca].T)
    t0 = time.perf_counter()
    za, zb, res, ncyc = _g.solve_zvector(_SpinView(scf, s), wvoa, wvob, cphf_conv_tol, cphf_max_cycle,
                                         vresp=None if xc is None else xc.vresp)
    tm["zvector_s"] = time.perf_counter() - t0
    tm["zvector_cycles"], tm["zvector_residual"] = ncyc, float(res)
    z1ao = np.asarray([orbva @ za @ orboa.T, orbvb @ zb @ orbob.T])
    zs = (z1ao + z1ao.transpose(0, 2, 1)) * 0.5
    if xc is None:
        vjz, vkz = get_jk(zs)
        veff = (vjz[0] + vjz[1])[None] - vkz
    else:
        veff = xc.vresp(zs)      # J - hyb K + V^resp[Z^S]
    # energy-weighted density W
    im0a = np.zeros_like(fockamo)
    im0b = np.zeros_like(fockbmo)
    im0a[:nocca, :nocca] = (fockamo[:nocca, :nocca] + orboa.T @ (veff0dooa + veff[0]) @ orboa
                            + ta @ fockamo[:nocca, :nocca] - x_ab.T @ vkmo[noccb:, :nocca])
    im0b[:noccb, :noccb] = fockbmo[:noccb, :noccb] + orbob.T @ (veff0doob + veff[1]) @ orbob
    im0b[noccb:, noccb:] = tb @ fockbmo[noccb:, noccb:].T - x_ab @ vkmo[noccb:, :nocca].T
    im0a[nocca:, :nocca] = za @ fockamo[:nocca, :nocca].T
    im0b[noccb:, :noccb] = zb @ fockbmo[:noccb, :noccb].T - 2.0 * x_ab @ vkmo[:noccb, :nocca].T
    im0 = mo_coeff[0] @ im0a @ mo_coeff[0].T + mo_coeff[1] @ im0b @ mo_coeff[1].T
    # relaxed difference densities T + Z^S and the ground state
    dmz1dooa, dmz1doob = zs[0] + dmta, zs[1] + dmtb
    oo0a, oo0b = orboa @ orboa.T, orbob @ orbob.T
    t0 = time.perf_counter()
    de = _g.contract_1e(mol, _g.hcore_generator(mol), _g.get_ovlp(mol), oo0a + oo0b + dmz1dooa + dmz1doob, im0)
    tm["one_electron_s"] = time.perf_counter() - t0
    # two-electron part: ground state + (T + Z^S) cross terms as D x D - TZ x TZ, and X_S, X_A
    da, db = oo0a + dmz1dooa, oo0b + dmz1doob
    tz = dmz1dooa + dmz1doob
    terms = [_g.jk_terms(1, 0, da + db, da + db), _g.jk_terms(-1, 0, tz, tz)]
    kw = hyb if rsh is None else 1.0     # range-separated: the pairs of full exchange, weighted per operator below
    if kw != 0:
        terms += [_g.jk_terms(0, -kw, da, da), _g.jk_terms(0, kw, dmz1dooa, dmz1dooa),
                  _g.jk_terms(0, -kw, db, db), _g.jk_terms(0, kw, dmz1doob, dmz1doob),
                  _g.jk_terms(0, -2 * kw, dmSx, dmSx),
                  (0.0, 2.0 * kw, dmAx - dmAx.T, dmAx)]        # -2 hyb vk[X_A] . (X_A[p,q] - X_A[q,p])
    # one xt_grad_jk call; range-separated: the same pairs as two lists, 2 Coulomb and 6 exchange pairs, two calls
    de += _g.grad_2e(mol, device, tm, hyb, rsh, terms=terms)
    if xc is not None:
        de += xc.grad((oo0a, oo0b), (dmz1dooa, dmz1doob))
    return de


class _SpinView:
    """The SCF object with its spin labels in the order ``s`` (what solve_zvector reads)."""

    def __init__(self, scf, s):
        self._scf = scf
        self.mo_coeff = [scf.mo_coeff[s[0]], scf.mo_coeff[s[1]]]
        self.mo_occ = [scf.mo_occ[s[0]], scf.mo_occ[s[1]]]
        self.mo_energy = [scf.mo_energy[s[0]], scf.mo_energy[s[1]]]
        self._veff = [scf._veff[s[0]], scf._veff[s[1]]]

    def get_hcore(self):
        return self._scf.get_hcore()

    def get_jk(self, dm=None, hermi=1):
        return self._scf.get_jk(dm=dm, hermi=hermi)


class SFGradients(_c.TDAGradients):
    """``SF_TDA_down(mf).nuc_grad_method()`` / ``SF_TDA_up(mf).nuc_grad_method()`` with the
    reference's attributes (usfcis.py:261-331; ``grad_common.TDAGradients``).
    A UHF reference takes method = 0; a UKS reference (LDA / GGA, pure or global hybrid, on a device)
    takes the collinear kernel, method = 2.  ``timings`` of the last gradient: ``one_electron_s``,
    ``grad_jk_s``, ``zvector_s`` / ``zvector_cycles`` / ``zvector_residual`` and, for a UKS reference,
    ``xc_response_s`` (every V^resp / wv evaluation, the Z-vector's included), ``grad_xc_s``."""

    _name, _not_run = "SF-TDA", RuntimeError
    _multicollinear = False      # SFU_gradient / SFD_gradient: method = 1 is accepted

    def __init__(self, td, *, allow_rsh=False):
        super().__init__(td, *_scf_of(td, self._multicollinear, allow_rsh))
        # the multicollinear kernel is differentiated at the sample count the roots were computed with
        self.collinear_samples = None
        if td.method == 1:
            from .sf_tda import DAVIDSON_SAMPLES, EXPLICIT_SAMPLES
            self.collinear_samples = int(td.collinear_samples or (DAVIDSON_SAMPLES if td.davidson else EXPLICIT_SAMPLES))

    def _davidson(self):
        return self.base.davidson

    def _amplitudes(self):
        return sf_amplitude(self.base, self.state - 1)

    def _ks_terms(self):
        td = self.base
        mc = dict(mf=td.mf, samples=self.collinear_samples) if td.method == 1 else None
        return KSTerms(self._scf, (1, 0) if td.isf == 1 else (0, 1), self.timings, self.xc_chunk, mc=mc)

    def _grad_elec(self, x, device, **kw):
        return grad_elec(self._scf, x, self.base.isf == 1, device, self.cphf_conv_tol, self.cphf_max_cycle,
                         self.timings, **kw)


class _SFKernelGradient(SFGradients):
    """``SFU_gradient`` / ``SFD_gradient``: the reference's entry to the spin-flip TDA gradient on a UKS
    reference (grad_hb/tduks_sfu.py ``SFU_gradient(td, method=1, state=1)``), which names the kernel."""

    _multicollinear = True
    _td_class = None

    def __init__(self, td, method=1, state=1, *, allow_rsh=False):
        from . import sf_tda
        want = getattr(sf_tda, self._td_class)
        if not isinstance(td, want):
            raise TypeError(f"{type(self).__name__} takes an {self._td_class} object, not {type(td).__name__}")
        if method != td.method:
            raise ValueError(f"{type(self).__name__}: method = {method}, but the roots were computed with "
                             f"method = {td.method}")
        if method == 0:
            raise NotImplementedError("spin-flip gradients with the ALDA0 kernel (method = 0) are not built "
                                      "(grad_hb/tduks_sfu.py raises likewise); methods 1 and 2 are")
        super().__init__(td, allow_rsh=allow_rsh)
        self.method = method
        self.state = state

    def kernel(self, atmlst=None):
        return super().kernel(None, atmlst)


class SFU_gradient(_SFKernelGradient):
    """Gradient of a spin-flip-up TDA state on a UKS reference (LDA / GGA, pure or global hybrid, on a
    device): ``SFU_gradient(td, method=1, state=1).kernel()`` with ``td`` an ``SF_TDA_up`` whose
    ``kernel()`` has run and ``method`` equal to ``td.method``.  method = 1 is the multicollinear kernel
    (DESIGN section 18), method = 2 runs exactly what ``td.nuc_grad_method()`` runs, method = 0 is not
    built.  The multicollinear kernel is differentiated at the sample count the roots were computed
    with (``collinear_samples``), not at the reference's fixed 20: only then is the result the
    derivative of the printed energy.

    Why two entries: ``nuc_grad_method()`` is pinned to refuse method = 1 (and stays the entry for
    Hartree-Fock references and the collinear kernel); the multicollinear gradient comes in under the
    name the reference gives it.  Attributes as ``SFGradients``; ``timings`` gains ``mc_kernel_grad_s``
    (the autograd pass of ``mcol.sf_mc_kernel_grad``) and ``xc_sf_response_s`` (``xt_xc_resp_sf`` /
    ``xt_xc_rows`` with their GEMMs)."""
    _td_class = "SF_TDA_up"


class SFD_gradient(_SFKernelGradient):
    """``SFU_gradient`` for a spin-flip-down state (``td`` an ``SF_TDA_down``): the same derivation with
    the spin labels exchanged.  The reference's ``SFD_gradient`` is an empty stub; this one works."""
    _td_class = "SF_TDA_down"
