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
which builds the same objects with ``allow_rsh=True``: every K above is hyb K + (alpha - hyb) K_LR (the one
``get_jk`` closure of ``grad_elec`` and ``qc.grad.ks_response``), and the kernel pairs go as two lists through
``xt_grad_jk2`` and ``xt_grad_jk2_lr`` (``qc.grad.grad_jk_rsh``).  ``nuc_grad_method()``, ``SFU_gradient(td)`` and
``SFD_gradient(td)`` with default arguments keep refusing them.
"""
from __future__ import annotations

import time

import numpy as np

from .qc import grad as _g


def _scf_of(td, multicollinear=False, allow_rsh=False):
    """(the SCF object behind ``td.mf``, whether it is a Kohn-Sham reference) after every refusal.
    ``multicollinear``: the caller is ``SFU_gradient`` / ``SFD_gradient``, which take method = 1;
    ``allow_rsh``: the caller came through ``.Gradients()``, which takes range-separated hybrids."""
    mf = td.mf
    if getattr(mf, "is_rohf", False):
        raise NotImplementedError("spin-flip gradients need a UHF / UKS reference (the reference's "
                                  "usfcis-rohf.py is not a working code path; tdroks_sfu.py is not built)")
    ref = mf.extra.get("qc_scf") if hasattr(mf, "extra") else None
    scf = ref() if ref is not None else None          # a weak reference: the mean field does not own the SCF
    if scf is None:
        if str(getattr(mf, "xctype", "HF")) != "HF":
            raise NotImplementedError(f"spin-flip gradients for xc = {mf.xc!r} need the qc UKS object the mean "
                                      "field came from (UKS.to_meanfield()), still alive")
        raise ValueError("the gradient needs the SCF object the mean field came from (qc UHF.to_meanfield()), "
                         "still alive")
    if str(getattr(scf, "xc", "HF")).upper() == "HF":
        if td.method != 0:
            raise NotImplementedError("spin-flip gradients on a Hartree-Fock reference are built for method = 0 only")
        _g.check_gradient_mf(scf)
        return scf, False
    if getattr(scf, "_device", None) is None:
        raise NotImplementedError(f"spin-flip gradients for xc = {scf.xc!r} on the host: the XC derivative "
                                  "(xt_grad_xc) and the XC response (xt_xc_resp) have no host path; call "
                                  "mf.to_device() before the SCF")
    _g.check_ks_gradient_mf(scf, allow_rsh=allow_rsh)
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


class KSTerms:
    """The XC hook of ``grad_elec`` for a UKS reference (LDA / GGA, collinear kernel): the response
    potential V^resp of the reference (``DeviceEngine.fxc_response``) and the XC nuclear-derivative
    terms (``qc.grad.grad_xc_pairs``).  ``grad_elec`` works in the labels "a" = flipped-from,
    "b" = flipped-to; the engine keeps alpha, beta, so every density pair is put into the engine's
    order on the way in and every potential back on the way out (``s``)."""

    def __init__(self, scf, s, timings, xc_chunk=None, mc=None):
        """``mc``: None for the collinear kernel; for the multicollinear one a dict
        with ``mf`` (the mean field of the TDA object) and ``samples`` (the sample count its roots were
        computed with)."""
        self.scf, self.s, self.tm = scf, s, timings
        self.mc = mc
        self.x_s = self.wv1 = self.wv2 = None      # multicollinear: X_S, wv1 (4, G), wv2 (2, 4, G) alpha, beta
        self.eng = scf.device_engine
        if self.eng is None:
            raise RuntimeError("the XC terms run on the GPU: run the SCF after mf.to_device()")
        self.xc_chunk = xc_chunk
        self.de_xc = None        # the XC nuclear-derivative part, set by grad()
        self._ks = _g.ks_response(scf)
        self.tm["xc_response_s"] = 0.0
        self.tm["xc_response_calls"] = 0

    def _order(self, pair):
        return np.asarray([pair[self.s[0]], pair[self.s[1]]])     # s is its own inverse

    def _timed(self, f, *a, **kw):
        t0 = time.perf_counter()
        out = f(*a, **kw)
        self.tm["xc_response_s"] += time.perf_counter() - t0
        self.tm["xc_response_calls"] += 1
        return out

    def vxc_resp(self, dm):
        """V^resp (2, nao, nao) of a symmetric density pair, in the labels of ``grad_elec``."""
        return self._order(self._timed(self.eng.fxc_response, self._order(dm), want=("v",))["v"])

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
        nk = 4 if eng.xctype == "GGA" else 1
        # rho0 through the engine's own GEMM (a fixed summation order): equal calls give equal bits
        with torch.cuda.device(eng.dev):
            rho0 = eng.rho(np.asarray([c[:, o > 0] @ c[:, o > 0].T for c, o in zip(self.scf.mo_coeff, self.scf.mo_occ)]))
        _, dq = sf_mc_kernel_grad(mf, out["rho1"][:nk], ns, device=eng.dev.index, rho=rho0)
        wv2 = torch.zeros((2, 4, out["wv"].shape[1]), dtype=torch.float64, device=eng.dev)
        wv2[:, :nk] = torch.as_tensor(dq, device=eng.dev) * eng.w
        torch.cuda.synchronize(eng.dev)
        self.tm["mc_kernel_grad_s"] = time.perf_counter() - t0
        self.x_s, self.wv1, self.wv2 = np.asarray(x_s), out["wv"], wv2
        return out["v"]

    def vxc_resp_t(self, dm):
        """What joins ``veff0doo``: f^xc[T], and with the multicollinear kernel V^k, the potential of
        wv2, from the same row pass (potentials are linear in their weights)."""
        if self.mc is None:
            return self.vxc_resp(dm)
        wv = self._timed(self.eng.fxc_response, self._order(dm), want=("wv",))["wv"]
        t0 = time.perf_counter()
        v = self.eng.rows_potential(wv + self.wv2)
        self.tm["xc_sf_response_s"] += time.perf_counter() - t0
        return self._order(v)

    def vresp(self, dm):
        """J[dm_a + dm_b] - hyb K[dm_s] + V^resp_s[dm]: what the Z-vector equations apply."""
        t0 = time.perf_counter()
        out = self._order(self._ks(self._order(dm)))
        self.tm["xc_response_s"] += time.perf_counter() - t0     # J / K included: one call of the response
        self.tm["xc_response_calls"] += 1
        return out

    def grad(self, d0, tz):
        """G_xc[w vxc[rho0]; D0 + T + Z^S] + G_xc[wv[T + Z^S]; D0], (natm, 3); d0, tz in the labels of
        ``grad_elec``.  With the multicollinear kernel wv2 joins wv[T + Z^S] and 2 G_xc[wv1; X_S] is
        added: a one-channel term, run as a two-spin pair whose second channel is zero."""
        import torch
        from .qc import xc as _xc
        eng = self.eng
        d0, tz = self._order(d0), self._order(tz)
        wv = self._timed(eng.fxc_response, tz, want=("wv",))["wv"]
        t0 = time.perf_counter()
        with torch.cuda.device(eng.dev):
            h0 = _xc.eval_xc_eff_torch(self.scf.xc, eng.rho(d0), deriv=1)[1] * eng.w
        st = {}
        pairs = [(h0, d0 + tz), (wv, d0)]
        if self.mc is not None:
            h1 = torch.zeros_like(self.wv2)
            h1[0] = 2.0 * self.wv1
            pairs = [(h0, d0 + tz), (wv + self.wv2, d0), (h1, np.asarray([self.x_s, np.zeros_like(self.x_s)]))]
        de = _g.grad_xc_pairs(self.scf, pairs, chunk=self.xc_chunk, stats=st)
        self.tm["grad_xc_s"] = time.perf_counter() - t0
        self.tm["grad_xc_stats"] = st
        self.de_xc = de
        return de


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

    k_lr = 0.0 if rsh is None else float(rsh[1]) - hyb

    def get_jk(dms):             # J / K do not depend on which spin a density belongs to
        dms = np.asarray(dms)
        if k_lr != 0:            # hyb K + (alpha - hyb) K_LR; get_k_lr takes non-symmetric densities
            vk_lr = k_lr * np.asarray(scf.get_k_lr(dms))
            if hyb == 0:
                return scf.get_jk(dm=dms, hermi=0, with_k=False)[0], vk_lr
            vj, vk = scf.get_jk(dm=dms, hermi=0)
            return vj, hyb * vk + vk_lr
        if hyb == 0:             # a pure functional forms no exchange
            return scf.get_jk(dm=dms, hermi=0, with_k=False)[0], np.zeros_like(dms)
        vj, vk = scf.get_jk(dm=dms, hermi=0)
        return vj, (vk if hyb == 1 else hyb * vk)

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
    t0 = time.perf_counter()
    st = {}
    if rsh is None:
        de += _g.grad_jk_device(mol, terms, device, stats=st)
    else:                        # the same pairs as two lists: 2 Coulomb and 6 exchange pairs, two calls
        jl, kl = _g.pair_lists(terms)
        de += _g.grad_jk_rsh(mol, jl, kl, float(rsh[0]), hyb, float(rsh[1]), device, stats=st)
        tm["grad_jk_full_s"], tm["grad_jk_lr_s"] = st.get("full_s"), st.get("lr_s")
        tm["buckets_lr"] = st.get("buckets_lr", [])
    tm["grad_jk_s"] = time.perf_counter() - t0
    tm["buckets"] = st.get("buckets", [])
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


class SFGradients:
    """``SF_TDA_down(mf).nuc_grad_method()`` / ``SF_TDA_up(mf).nuc_grad_method()`` with the
    reference's attributes (usfcis.py:261-331): ``state`` (1-based), ``cphf_conv_tol``,
    ``cphf_max_cycle`` (the values its solver actually runs with, usfcis.py:145-148), ``atmlst``.
    A UHF reference takes method = 0; a UKS reference (LDA / GGA, pure or global hybrid, on a device)
    takes the collinear kernel, method = 2.  ``timings`` of the last gradient: ``one_electron_s``,
    ``grad_jk_s``, ``zvector_s`` / ``zvector_cycles`` / ``zvector_residual`` and, for a UKS reference,
    ``xc_response_s`` (every V^resp / wv evaluation, the Z-vector's included), ``grad_xc_s``."""

    cphf_max_cycle = 500
    cphf_conv_tol = 1e-10

    _multicollinear = False      # SFU_gradient / SFD_gradient: method = 1 is accepted

    def __init__(self, td, *, allow_rsh=False):
        self.base = td
        self._scf, self.is_ks = _scf_of(td, self._multicollinear, allow_rsh)
        # the multicollinear kernel is differentiated at the sample count the roots were computed with
        self.collinear_samples = None
        if td.method == 1:
            from .sf_tda import DAVIDSON_SAMPLES, EXPLICIT_SAMPLES
            self.collinear_samples = int(td.collinear_samples or (DAVIDSON_SAMPLES if td.davidson else EXPLICIT_SAMPLES))
        self.mol = self._scf.mol
        self.state = 1
        self.atmlst = None
        self.de = None
        self.de_xc = None        # the XC nuclear-derivative part of the last gradient (UKS reference)
        self.xc_chunk = None     # grid points per xt_grad_xc call; None: qc.grad.default_xc_chunk
        self.timings = {}

    def grad_nuc(self, mol=None, atmlst=None):
        return _g.grad_nuc(mol or self.mol, atmlst)

    def grad_elec(self, atmlst=None):
        td = self.base
        if getattr(td, "v", None) is None:
            raise RuntimeError("run the SF-TDA kernel() first")
        if not 1 <= self.state <= np.asarray(td.v).shape[1]:
            raise ValueError(f"state {self.state} is not among the computed roots")
        conv = getattr(td, "converged", None)
        if td.davidson and conv is not None and not bool(np.asarray(conv)[self.state - 1]):
            raise RuntimeError(f"root {self.state} of the Davidson solve is not converged")
        dev = getattr(self._scf, "_device", None)
        if dev is None:
            raise RuntimeError("the gradient runs on the GPU (xt_grad_jk, device J / K): call "
                               "mf.to_device() before the SCF")
        flip = td.isf == 1
        if self.is_ks:
            self.timings.clear()
            mc = dict(mf=td.mf, samples=self.collinear_samples) if td.method == 1 else None
            xc = KSTerms(self._scf, (1, 0) if flip else (0, 1), self.timings, self.xc_chunk, mc=mc)
            omega = float(getattr(self._scf, "omega", 0.0))
            rsh = (omega, float(self._scf.alpha)) if omega != 0 else None
            root = float(np.asarray(td.e)[self.state - 1]) if rsh is not None else None
            de = grad_elec(self._scf, sf_amplitude(td, self.state - 1), flip, dev, self.cphf_conv_tol,
                           self.cphf_max_cycle, self.timings, hyb=float(self._scf.hyb), xc=xc, rsh=rsh, root=root)
            self.de_xc = xc.de_xc
        else:
            de = grad_elec(self._scf, sf_amplitude(td, self.state - 1), flip, dev, self.cphf_conv_tol,
                           self.cphf_max_cycle, self.timings)
        return de if atmlst is None else de[list(atmlst)]

    def kernel(self, state=None, atmlst=None):
        if state is not None:
            self.state = state
        if atmlst is None:
            atmlst = self.atmlst
        else:
            self.atmlst = atmlst
        self.de = self.grad_elec(atmlst) + self.grad_nuc(atmlst=atmlst)
        return self.de


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
