"""Host checks of the UKS ground-state gradient (no GPU): the closed-form AO second derivatives
of the restatement ``tests/ksgrad_ref.py`` against central differences of ``Mole.eval_ao``, the
restated gradient against finite differences of host UKS energies on a grid frozen in space, the
argument checks of the C entry ``xt_grad_xc`` and the refusals of ``KSGradients``.

Frozen grid: every displaced SCF gets the undisplaced ``Grids`` object, so the energy is a smooth
function of the nuclei whose derivative is exactly the ``grid_response = False`` gradient; a coarse
grid (``ksgrad_ref.coarse_grids``) therefore serves.  Translational invariance of the XC part does not hold on such a grid and
is not asserted; sum_A g[A] is printed as a diagnostic of the grid."""
import os

import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
from xtddft_amd import _capi, build, qc
from xtddft_amd.qc import grad as G

EPS = np.finfo(np.float64).eps
H_FD = 2e-3       # Bohr
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # the bent geometry of tests/test_gpu_grad.py (Angstrom)

# a contracted s and p, and d / f / g shells on three non-collinear centres
SPDFG = {"H": [[0, [4.0, 0.11], [1.1, 0.52], [0.35, 0.48]], [1, [1.3, 0.4], [0.5, 0.7]], [2, [0.7, 1.0]],
               [3, [0.9, 1.0]], [4, [0.8, 1.0]]]}
ATOMS = [("H", (0.0, 0.0, 0.0)), ("H", (0.0, 1.7, 1.1)), ("H", (1.3, -0.9, 0.6))]


# --------------------------------------------------------------------------- AO second derivatives
def test_ao_second_derivatives_against_central_differences():
    """The restatement's value and first derivatives equal ``eval_ao(deriv=1)`` to rounding; its
    second derivatives d_j d_i phi are checked against central differences of the host d_i phi in
    the grid coordinate j: two Richardson estimates from the steps (2h, h) and (h, h/2), bound
    10 x their difference + 24 eps max|grad phi| / h.  The rounding term: the host ``eval_ao`` is
    held to 16 2^-53 = 8 eps of its scale (tests/test_int_cases.py), a central difference at
    step s divides two such errors by 2s, and R(h, h/2) = (4 d(h/2) - d(h)) / 3 adds them with the
    weights 4/3 and 1/3: (4 / (h/2) + 1 / h) / 3 x 8 eps = 24 eps / h."""
    mol = qc.M(ATOMS, basis=SPDFG, spin=1, unit="Bohr")
    assert sorted({s.l for s in mol.shells}) == [0, 1, 2, 3, 4] and max(s.exps.size for s in mol.shells) == 3
    rng = np.random.default_rng(5)
    coords = np.concatenate([np.asarray(c)[None] + rng.uniform(-1.5, 1.5, (12, 3)) for _, c in ATOMS])
    ao10 = K.ao_deriv2(mol, coords)
    host = np.asarray(mol.eval_ao(coords, deriv=1))
    scale = np.abs(host[1:]).max()
    assert np.abs(ao10[:4] - host).max() <= 64 * EPS * np.abs(host).max()
    for j in range(3):
        step = np.zeros(3)
        step[j] = 1.0
        fine, coarse = R.richardson(lambda s: np.asarray(mol.eval_ao(coords + s * step, deriv=1))[1:], H_FD)
        for i in range(3):
            ana = ao10[4 + K.PAIR_INDEX[i, j]]
            lhs = np.abs(ana - fine[i]).max()
            rhs = 10 * np.abs(fine[i] - coarse[i]).max() + 24 * EPS * scale / H_FD
            print(f"d{'xyz'[j]} d{'xyz'[i]} phi: max|closed form - FD| = {lhs:.2e} <= {rhs:.2e}")
            assert lhs <= rhs, (i, j, lhs, rhs)


# --------------------------------------------------------------------------- restated gradient
def run_uks(mol, xc, grids, conv_tol=1e-12):
    mf = qc.UKS(mol, xc=xc)
    mf.grids = grids                 # build() keeps a grid that is already set
    mf.conv_tol = conv_tol
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.kernel()
    assert mf.converged
    return mf


@pytest.mark.parametrize("xc", ["svwn", "b3lyp"])
def test_restated_uks_gradient_against_frozen_grid_finite_differences(xc):
    """CH2 / 6-31G, LDA (SVWN) and B3LYP on a coarse grid (every eighth point of the level-3
    grid) frozen in space, one random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, 8)
    mf = run_uks(mol, xc, grids)
    g, S, parts = K.uks_grad(mf)
    u = R.random_direction(mol.natm, 1)
    runs = {}
    for s in (2 * H_FD, H_FD, H_FD / 2):
        for sg in (1, -1):
            m = run_uks(R.displaced(mol, u, sg * s), xc, grids)
            assert m.grids is grids
            runs[sg * s] = (m.e_tot, m.last_energy_change)
    eps_e = max([mf.last_energy_change] + [v[1] for v in runs.values()])
    fine, coarse = R.richardson(lambda s: runs[s][0], H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"UKS {xc} ({grids.size} points): g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} "
          f"<= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e}); S = {S:.3e}, "
          f"max|g_xc| = {np.abs(parts['xc']).max():.3e}, sum_A g = {parts['sum_atoms']}")
    assert np.abs(parts["xc"]).max() > 1e-3            # the XC term is a real part of what is checked
    assert lhs <= rhs


# --------------------------------------------------------------------------- the C entry
def test_exports_and_build_lists():
    assert "xt_grad_xc" in _capi.EXPORTS
    assert "xt_grad_xc.hip" in build.SOURCES
    assert _capi.ABI_VERSION == 8                      # a pure addition: no bump
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        assert "int xt_grad_xc(" in f.read()
    assert G.xc_work_size(65, 3) == 3 * 3 * 3 and G.xc_work_size(64, 3) == 3 * 3 * 2


def test_xt_grad_xc_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with its own message before the first HIP call."""
    L = hiplib
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data

    def call(ngrid=1, coords=d, nshell=1, info=i, dat=d, sph=d, norm=d, atom=i, lmax=0, natm=1, nao=1, nspin=2,
             xctype=_capi.XC["GGA"], h=d, e=d, c=d, ldg=1, work=d, nwork=6, out=d):
        return L.xt_grad_xc(ngrid, coords, nshell, info, dat, sph, norm, atom, lmax, natm, nao, nspin, xctype, h, e, c,
                            ldg, work, nwork, out, None)

    def rejected(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.xt_last_error(), L.xt_last_error()
    for name in ("ngrid", "nshell", "natm", "nao", "ldg", "nwork"):
        rejected(call(**{name: -1}), "negative size")
    rejected(call(lmax=5), "lmax")
    rejected(call(lmax=-1), "lmax")
    for nspin in (0, 3):
        rejected(call(nspin=nspin), "nspin")
    for flag in (_capi.XC["HF"], _capi.XC["MGGA"], 7):
        rejected(call(xctype=flag), "xctype")
    rejected(call(ngrid=2, ldg=1, nwork=6), "ldg")
    rejected(call(nwork=5), "workspace")
    rejected(call(ngrid=65, ldg=65, nwork=8), "workspace")          # two tiles + 1: 9 doubles
    rejected(call(ngrid=2**31 - 1, ldg=2**31 - 1, nshell=2**31 - 1, nwork=2**62), "blocks")
    for name in ("coords", "info", "dat", "sph", "norm", "atom", "e", "work", "out"):
        rejected(call(**{name: None}), "null")
        rejected(call(**{name: None}, xctype=_capi.XC["LDA"]), "null")
    for name in ("h", "c"):
        rejected(call(**{name: None}), "needs h and c")
    assert call(ngrid=0, coords=None, e=None) == 0 and call(nshell=0, info=None, nwork=0) == 0   # nothing to add
    assert call(natm=0, out=None) == 0


# --------------------------------------------------------------------------- refusals
def test_refusals():
    from xtddft_amd.sf_tda import SF_TDA_down
    mol = qc.M(CH2, basis="6-31g", spin=2)
    for make in (lambda: qc.UKS(mol, xc="tpss"), lambda: qc.UKS(mol, xc="cam-b3lyp"),
                 lambda: qc.UKS(mol, xc="b3lyp", nlc=(6.0, 0.01)), lambda: qc.ROKS(mol, xc="b3lyp"),
                 lambda: qc.UKS(mol, xc="b3lyp").density_fit(), lambda: qc.UKS(mol, xc="b3lyp").sfx2c1e()):
        mf = make().to_device(0)
        with pytest.raises(NotImplementedError):
            mf.nuc_grad_method()
    loose = qc.UKS(mol, xc="pbe").to_device(0)
    loose.eri_mode, loose.chol_tol = "cholesky", 1e-6
    with pytest.raises(ValueError):
        loose.nuc_grad_method()
    for xc in ("svwn", "pbe", "b3lyp"):
        gm = qc.UKS(mol, xc=xc).to_device(0).nuc_grad_method()
        assert isinstance(gm, G.KSGradients) and gm.grid_response is False
        gm.grid_response = False
        with pytest.raises(NotImplementedError):
            gm.grid_response = True
    with pytest.raises(NotImplementedError):       # no host path for the XC derivative
        qc.UKS(mol, xc="b3lyp").nuc_grad_method()
    assert type(qc.UHF(mol).to_device(0).nuc_grad_method()) is G.Gradients
    with pytest.raises(NotImplementedError):       # check_gradient_mf is unchanged
        G.check_gradient_mf(qc.UKS(mol, xc="b3lyp").to_device(0))
    uks = qc.UKS(mol, xc="b3lyp")
    uks.kernel()
    with pytest.raises(NotImplementedError):       # the spin-flip CIS gradients still refuse a UKS reference
        SF_TDA_down(uks.to_meanfield(), davidson=False).nuc_grad_method()
    assert len(G.ks_ground_terms(np.eye(2), np.eye(2), 0.0)) == 1 and len(G.ks_ground_terms(np.eye(2), np.eye(2), 0.2)) == 3
