"""Host checks of the collinear spin-flip TDA gradient on a UKS reference (no GPU): the NumPy
restatement ``tests/sfksgrad_ref.py`` against finite differences of host energies on a grid frozen
in space and against the spin-flip CIS restatement in the Hartree-Fock limit, the argument checks of
the C entry ``xt_xc_resp``, its export lists, and the refusals of the driver.

Frozen grid: every displaced SCF gets the undisplaced ``Grids`` object, as in
``tests/test_ksgrad_host.py``; translational invariance does not hold on such a grid and sum_A g[A] is
printed only."""
import os

import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
import sfksgrad_ref as SK
from xtddft_amd import _capi, build, qc
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up

H_FD = 2e-3       # Bohr
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # the bent geometry of tests/test_gpu_grad.py (Angstrom)
GAP = 1e-3        # Ha: the root is separated from its neighbours by more than this


def run_uks(mol, xc, grids, conv_tol=1e-12):
    mf = qc.UKS(mol, xc=xc)
    mf.grids = grids                 # build() keeps a grid that is already set
    mf.conv_tol = conv_tol
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.kernel()
    assert mf.converged
    return mf


def _xao(mf, x, isf):
    s = (0, 1) if isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    return np.asarray([cv @ xi @ co.T for xi in np.atleast_3d(x).reshape(-1, cv.shape[1], co.shape[1])])


def _separated(e, k):
    nb = [abs(e[k] - e[j]) for j in (k - 1, k + 1) if 0 <= j < e.size]
    return min(nb)


# --------------------------------------------------------------------------- restated gradient
@pytest.fixture(scope="module")
def fd_runs():
    """Per functional: the undisplaced UKS and the six displaced ones of one random direction, all on
    the same coarse frozen grid."""
    out = {}

    def get(xc):
        if xc not in out:
            mol = qc.M(CH2, basis="6-31g", spin=2)
            grids = K.coarse_grids(mol, 8)
            mf = run_uks(mol, xc, grids)
            u = R.random_direction(mol.natm, 1)
            runs = {}
            for s in (2 * H_FD, H_FD, H_FD / 2):
                for sg in (1, -1):
                    m = run_uks(R.displaced(mol, u, sg * s), xc, grids)
                    assert m.grids is grids
                    runs[sg * s] = m
            out[xc] = (mol, mf, u, runs, R.deriv_eri(mol), SK.xc_arrays(mf), {})
        return out[xc]
    return get


@pytest.mark.parametrize("isf", [-1, 1])
@pytest.mark.parametrize("xc", ["b3lyp", "bhandhlyp"])
def test_restated_gradient_against_frozen_grid_finite_differences(fd_runs, xc, isf):
    """CH2 / 6-31G on every eighth point of the level-3 grid, frozen; state 1 of the collinear
    spin-flip-down and spin-flip-up A matrices (dense, from MO integrals), E = e_tot + omega, one
    random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr.
    The root is followed by the overlap of the AO transition densities and must stay more than 1e-3 Ha
    from its neighbours at every geometry; the part of the gradient that fxc enters must exceed
    1e-4 Ha / Bohr."""
    mol, mf, u, runs, ip, xa, mcache = fd_runs(xc)
    state = 0
    e0, xs0 = SK.sf_states(mf, isf)
    assert _separated(e0, state) > GAP, (e0[:4])
    g, S, parts = SK.sf_ks_grad(mf, xs0[state], isf, ip, xa, mcache=mcache)
    g_nofxc = SK.sf_ks_grad(mf, xs0[state], isf, ip, xa, with_fxc=False)[0]
    fxc_part = np.abs(g - g_nofxc).max()
    x0 = _xao(mf, xs0[state], isf)[0]

    def energy(s):
        m = runs[s]
        e, xs = SK.sf_states(m, isf)
        k, ov = R.follow(mf.s1e, x0, _xao(m, xs[:6], isf))
        assert ov > 0.9, (s, ov)
        assert _separated(e, k) > GAP, (s, e[:4])
        return m.e_tot + e[k]
    eps_e = max([mf.last_energy_change] + [m.last_energy_change for m in runs.values()])
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"SF {isf:+d} state 1 on UKS {xc} ({mf.grids.size} points): omega = {e0[state]:.6f} (gap "
          f"{_separated(e0, state):.2e}), g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= "
          f"{rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e}); S = {S:.3e}, max|fxc part| = "
          f"{fxc_part:.3e}, max|G_xc[wv; D0]| = {np.abs(parts['xc_fxc']).max():.3e}, sum_A g = {parts['sum_atoms']}")
    assert fxc_part > 1e-4
    assert lhs <= rhs


@pytest.mark.parametrize("isf", [-1, 1])
def test_restatement_reproduces_spin_flip_cis_in_the_hartree_fock_limit(isf):
    """Every XC array zero and hyb = 1 on a UHF reference: ``grad_ref.sf_grad`` to 1e-10, and the
    collinear A matrix from MO integrals has the spectrum of the oracle's explicit A."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    mf = R.run_uhf(mol)
    ip = R.deriv_eri(mol)
    e_ref, xs_ref, _ = R.sf_states(mf, isf)
    e, xs = SK.sf_states(mf, isf, hyb=1.0)
    assert np.abs(e - e_ref).max() <= 1e-10
    worst = 0.0
    for state in (0, 1):
        ref = R.sf_grad(mf, xs_ref[state], isf, ip)
        got, _, parts = SK.sf_ks_grad(mf, xs_ref[state], isf, ip, SK.zero_xc_arrays(mol.nao), hyb=1.0)
        assert np.abs(parts["xc"]).max() == 0.0
        worst = max(worst, np.abs(got - ref).max())
        # the restatement's own amplitude is the oracle's up to a sign
        assert abs(abs(float((xs[state] * xs_ref[state]).sum())) - 1.0) <= 1e-8
    print(f"SF {isf:+d}: max|restatement(hyb = 1, no XC) - spin-flip CIS restatement| = {worst:.2e}")
    assert worst <= 1e-10


# --------------------------------------------------------------------------- the C entry
def test_exports_and_build_lists():
    assert "xt_xc_resp" in _capi.EXPORTS
    assert "xt_xc_resp.hip" in build.SOURCES
    assert _capi.ABI_VERSION == 8                      # a pure addition: no bump
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        text = f.read()
    assert "int xt_xc_resp(" in text and "#define XT_ABI_VERSION 8" in text
    assert os.path.exists(os.path.join(root, "xtddft_amd", "csrc", "xt_xc_resp.hip"))


def test_xt_xc_resp_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with its own message before the first HIP call;
    the zero-size calls return 0."""
    L = hiplib
    buf = np.zeros(256)
    d = buf.ctypes.data

    def call(ngrid=2, nao=3, xctype=_capi.XC["GGA"], ao=d, ao_plane=6, ldao=3, c=d, ldc=3, fxc=d, ldg=2, w=d,
             rho1=d, wv=d, ldo=2, b=d, ldb=3):
        return L.xt_xc_resp(ngrid, nao, xctype, ao, ao_plane, ldao, c, ldc, fxc, ldg, w, rho1, wv, ldo, b, ldb, None)

    def rejected(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.xt_last_error(), L.xt_last_error()
    for name in ("ngrid", "nao", "ao_plane", "ldao", "ldc", "ldg", "ldo", "ldb"):
        rejected(call(**{name: -1}), "negative size")
    for flag in (_capi.XC["HF"], _capi.XC["MGGA"], 7):
        rejected(call(xctype=flag), "xctype")
    for name in ("ldao", "ldc", "ldb"):
        rejected(call(**{name: 2}), name)
        rejected(call(**{name: 2}, xctype=_capi.XC["LDA"]), name)
    rejected(call(ldg=1), "ldg")
    rejected(call(ldo=1), "ldo")
    rejected(call(ao_plane=5), "ao_plane")
    assert call(ao_plane=0, xctype=_capi.XC["LDA"], ao=None) == -1 and b"null" in L.xt_last_error()   # LDA: one plane
    rejected(call(ngrid=2**40, ldg=2**40, ldo=2**40, ao_plane=2**44), "blocks")
    for name in ("ao", "c", "fxc", "w"):
        rejected(call(**{name: None}), "null")
        rejected(call(**{name: None}, xctype=_capi.XC["LDA"]), "null")
    assert call(ngrid=0, ao=None, c=None, fxc=None, w=None, ldg=0, ldo=0, ao_plane=0) == 0
    assert call(nao=0, ao=None, c=None, fxc=None, w=None) == 0
    assert call(rho1=None, wv=None, b=None, ao=None) == 0                   # nothing asked for: nothing read


# --------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def host_scfs():
    """Converged host mean fields on a coarse grid (the refusals are decided before any device work),
    flagged as device mean fields afterwards where the case needs it."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, 8)

    def make(build, device=True):
        mf = build(mol)
        if str(mf.xc).upper() != "HF":
            mf.grids = grids
        mf.max_cycle = 300
        mf.kernel()
        assert mf.converged
        mfield = mf.to_meanfield()
        if device:
            mf.to_device(0)          # records the device only; the SCF itself ran on the host
        return mf, mfield
    return mol, make


def test_driver_refusals(host_scfs):
    mol, make = host_scfs
    uks, mfield = make(lambda m: qc.UKS(m, xc="b3lyp"))
    for method in (0, 1):
        with pytest.raises(NotImplementedError) as err:
            SF_TDA_down(mfield, method=method, davidson=False).nuc_grad_method()
        assert ("ALDA0", "multicollinear")[method] in str(err.value)
    for cls in (SF_TDA_down, SF_TDA_up):
        gm = cls(mfield, method=2, davidson=False).nuc_grad_method()      # accepted
        assert gm.is_ks and (gm.state, gm.cphf_conv_tol, gm.atmlst) == (1, 1e-10, None)
        with pytest.raises(RuntimeError):                                  # the TDA kernel() has not run
            gm.kernel()
    # a KS mean field on the host: no host path for the XC derivative, whatever the method
    host, hfield = make(lambda m: qc.UKS(m, xc="b3lyp"), device=False)
    for method in (0, 2):
        with pytest.raises(NotImplementedError) as err:
            SF_TDA_down(hfield, method=method, davidson=False).nuc_grad_method()
        assert "host" in str(err.value)
    # everything check_ks_gradient_mf refuses
    for build_mf in (lambda m: qc.ROKS(m, xc="b3lyp"), lambda m: qc.UKS(m, xc="tpss"),
                     lambda m: qc.UKS(m, xc="cam-b3lyp"), lambda m: qc.UKS(m, xc="b3lyp", nlc=(6.0, 0.01)),
                     lambda m: qc.UKS(m, xc="b3lyp").density_fit(), lambda m: qc.UKS(m, xc="b3lyp").sfx2c1e()):
        keep, field = make(build_mf)
        with pytest.raises(NotImplementedError):
            SF_TDA_down(field, method=2, davidson=False).nuc_grad_method()
    loose, lfield = make(lambda m: qc.UKS(m, xc="pbe"))
    loose.eri_mode, loose.chol_tol = "cholesky", 1e-6
    with pytest.raises(ValueError):
        SF_TDA_down(lfield, method=2, davidson=False).nuc_grad_method()
    # Hartree-Fock references behave as before: method 0 only
    hf, hffield = make(lambda m: qc.UHF(m))
    assert not SF_TDA_down(hffield, davidson=False).nuc_grad_method().is_ks
    for method in (1, 2):
        with pytest.raises(NotImplementedError):
            SF_TDA_down(hffield, method=method, davidson=False).nuc_grad_method()
