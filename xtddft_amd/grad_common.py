"""What the excited-state gradient drivers share on the host (``grad.py``: spin-flip TDA, ``grad_utda.py``:
U-TDA); the Lagrangians themselves are the ``grad_elec`` of either module.

* ``scf_behind`` / ``check_reference`` -- from the mean field of a TDA object to the qc SCF object it came from,
  and the refusals every driver shares (``qc.grad.check_gradient_mf`` / ``check_ks_gradient_mf``, a Kohn-Sham mean
  field on the host); each driver's ``_scf_of`` puts its own refusals around them;
* ``KSTerms`` -- the XC hook of ``grad_elec`` on a UKS reference (LDA / GGA): the timed response calls of the
  engine, the Z-vector's operator (``qc.grad.ks_response``), f^xc[T] with the kernel-derivative weights wv2 and the
  XC nuclear-derivative pairs (``qc.grad.grad_xc_pairs``).  A driver's subclass supplies the order of its spin
  labels, its coupling (which keeps ``x_s``, ``wv1``, ``wv2``) and its extra pair;
* ``TDAGradients`` -- the driver object with the reference's attributes (``state``, ``cphf_conv_tol``,
  ``cphf_max_cycle``, ``atmlst``), its checks, ``grad_nuc`` and ``kernel``.

The two-electron dispatch (``qc.grad.grad_2e``) and the exchange closure (``qc.grad.exchange_jk``) live with the
kernels' wrappers in ``qc/grad.py``.
"""
from __future__ import annotations

import time

import numpy as np

from .qc import grad as _g


def scf_behind(mf):
    """The qc SCF object the mean field came from (``to_meanfield()``), None when it is gone: the mean field
    holds a weak reference and does not own it."""
    ref = mf.extra.get("qc_scf") if hasattr(mf, "extra") else None
    return ref() if ref is not None else None


def is_hartree_fock(scf):
    return str(getattr(scf, "xc", "HF")).upper() == "HF"


def check_reference(scf, what, allow_rsh=False):
    """Whether ``scf`` is a Kohn-Sham reference, after the refusals of ``qc.grad`` and of a Kohn-Sham mean field
    on the host.  ``what`` names the driver in the message; ``allow_rsh``: the caller came through
    ``.Gradients()``, which takes range-separated hybrids."""
    if is_hartree_fock(scf):
        _g.check_gradient_mf(scf)
        return False
    if getattr(scf, "_device", None) is None:
        raise NotImplementedError(f"{what} gradients for xc = {scf.xc!r} on the host: the XC derivative "
                                  "(xt_grad_xc) and the XC response (xt_xc_resp) have no host path; call "
                                  "mf.to_device() before the SCF")
    _g.check_ks_gradient_mf(scf, allow_rsh=allow_rsh)
    return True


class KSTerms:
    """The XC terms of a ``grad_elec`` on a UKS reference (LDA / GGA).  The engine keeps alpha, beta; a driver
    that works in other labels overrides ``_order``, which takes a pair into the engine's order on the way in
    and, being its own inverse, a potential back on the way out.  ``x_s``, ``wv1`` and ``wv2`` are set by the
    subclass's coupling: wv2 (2, 4, G), the density derivative of the kernel's energy, joins wv[T] and
    wv[T + Z^S]; ``extra_pairs`` is the G_xc pair of wv1 with ``x_s``."""

    def __init__(self, scf, timings, xc_chunk=None):
        self.scf, self.tm = scf, timings
        self.eng = scf.device_engine
        if self.eng is None:
            raise RuntimeError("the XC terms run on the GPU: run the SCF after mf.to_device()")
        self.xc_chunk = xc_chunk
        self.de_xc = None        # the XC nuclear-derivative part, set by grad()
        self.x_s = self.wv1 = self.wv2 = None
        self._ks = _g.ks_response(scf)
        self.tm["xc_response_s"] = 0.0
        self.tm["xc_response_calls"] = 0

    def _order(self, pair):
        return np.asarray(pair)

    def extra_pairs(self):
        return []

    def _timed(self, f, *a, **kw):
        t0 = time.perf_counter()
        out = f(*a, **kw)
        self.tm["xc_response_s"] += time.perf_counter() - t0
        self.tm["xc_response_calls"] += 1
        return out

    @property
    def nk(self):
        """Rows of rho the functional reads: the density and, for GGA, its gradient."""
        return 4 if self.eng.xctype == "GGA" else 1

    def _kernel_weights(self, dq):
        """w dq, the ``nk`` rows of the kernel's density derivative per spin, in the (2, 4, G) layout of the
        engine's weights."""
        import torch
        eng = self.eng
        wv2 = torch.zeros((2, 4, eng.w.shape[0]), dtype=torch.float64, device=eng.dev)
        wv2[:, :self.nk] = torch.as_tensor(dq, device=eng.dev) * eng.w
        return wv2

    def rho0(self):
        """The ground density on the grid, (2, 4, G), through the engine's own GEMM (a fixed summation order):
        equal calls give equal bits."""
        import torch
        with torch.cuda.device(self.eng.dev):
            return self.eng.rho(np.asarray([c[:, o > 0] @ c[:, o > 0].T
                                            for c, o in zip(self.scf.mo_coeff, self.scf.mo_occ)]))

    def vxc_resp(self, dm):
        """V^resp (2, nao, nao) of a symmetric density pair, in the labels of ``grad_elec``."""
        return self._order(self._timed(self.eng.fxc_response, self._order(dm), want=("v",))["v"])

    def vresp(self, dm):
        """J[dm_a + dm_b] - hyb K[dm_s] + V^resp_s[dm]: what the Z-vector equations apply; J / K included, it
        counts as one call of the response."""
        return self._order(self._timed(self._ks, self._order(dm)))

    def vxc_resp_t(self, dm):
        """What joins ``veff0doo``: f^xc[T] and the potential of wv2, from one row pass (potentials are linear
        in their weights); its seconds go to the subclass's ``_rows_done``."""
        wv = self._timed(self.eng.fxc_response, self._order(dm), want=("wv",))["wv"]
        t0 = time.perf_counter()
        v = self.eng.rows_potential(wv + self.wv2)
        self._rows_done(time.perf_counter() - t0)
        return self._order(v)

    def grad(self, d0, tz):
        """G_xc[w vxc[rho0]; D0 + T + Z^S] + G_xc[wv[T + Z^S] (+ wv2); D0] + the extra pairs, (natm, 3); d0, tz
        in the labels of ``grad_elec``."""
        import torch
        from .qc import xc as _xc
        eng = self.eng
        d0, tz = self._order(d0), self._order(tz)
        wv = self._timed(eng.fxc_response, tz, want=("wv",))["wv"]
        t0 = time.perf_counter()
        with torch.cuda.device(eng.dev):
            h0 = _xc.eval_xc_eff_torch(self.scf.xc, eng.rho(d0), deriv=1)[1] * eng.w
        st = {}
        if self.wv2 is not None:
            wv = wv + self.wv2
        pairs = [(h0, d0 + tz), (wv, d0)] + self.extra_pairs()
        de = _g.grad_xc_pairs(self.scf, pairs, chunk=self.xc_chunk, stats=st)
        self.tm["grad_xc_s"] = time.perf_counter() - t0
        self.tm["grad_xc_stats"] = st
        self.de_xc = de
        return de


class TDAGradients:
    """The gradient object of one TDA driver: ``state`` (1-based), ``cphf_conv_tol``, ``cphf_max_cycle`` (the
    values the reference's solver actually runs with, usfcis.py:145-148), ``atmlst``, ``xc_chunk``, ``de``,
    ``de_xc`` and ``timings`` of the last gradient.  A subclass names its driver (``_name``, ``_not_run``: the
    exception of a TDA object without roots), and provides ``_davidson()``, ``_amplitudes()``, ``_ks_terms()``
    and ``_grad_elec(x, device, **kw)``, the call into its module's ``grad_elec``."""

    cphf_max_cycle = 500
    cphf_conv_tol = 1e-10

    def __init__(self, td, scf, is_ks):
        self.base = td
        self._scf, self.is_ks = scf, is_ks
        self.mol = scf.mol
        self.state = 1
        self.atmlst = None
        self.de = None
        self.de_xc = None        # the XC nuclear-derivative part of the last gradient (UKS reference)
        self.xc_chunk = None     # grid points per xt_grad_xc call; None: qc.grad.default_xc_chunk
        self.timings = {}

    def grad_nuc(self, mol=None, atmlst=None):
        return _g.grad_nuc(mol or self.mol, atmlst)

    def grad_elec(self, atmlst=None):
        td, scf = self.base, self._scf
        if getattr(td, "v", None) is None:
            raise self._not_run(f"run the {self._name} kernel() first")
        if not 1 <= self.state <= np.asarray(td.v).shape[1]:
            raise ValueError(f"state {self.state} is not among the computed roots")
        conv = getattr(td, "converged", None)
        if self._davidson() and conv is not None and not bool(np.asarray(conv)[self.state - 1]):
            raise RuntimeError(f"root {self.state} of the Davidson solve is not converged")
        dev = getattr(scf, "_device", None)
        if dev is None:
            raise RuntimeError("the gradient runs on the GPU (derivative integrals and J / K on the device): call "
                               "mf.to_device() before the SCF")
        self.timings.clear()
        x = self._amplitudes()
        if self.is_ks:
            xc = self._ks_terms()
            omega = float(getattr(scf, "omega", 0.0))
            rsh = (omega, float(scf.alpha)) if omega != 0 else None
            root = float(np.asarray(td.e)[self.state - 1]) if rsh is not None else None
            de = self._grad_elec(x, dev, hyb=float(scf.hyb), xc=xc, rsh=rsh, root=root)
            self.de_xc = xc.de_xc
        else:
            de = self._grad_elec(x, dev)
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
