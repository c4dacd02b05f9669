"""VV10 (NLC) on the host: the front end's energy and potential, and the NumPy restatement of
the second derivative that the GPU tests compare the device against, both pinned to the one
stated energy formula (tests/vv10_ref.py: mpmath differences in point space, the complex step at
the AO level).  Parity with PySCF's get_vnlc_resp is NOT pinned anywhere: PySCF is not available
and the reference stores no VV10 output."""
import ctypes
import os

import numpy as np
import pytest

import vv10_ref as ref
from xtddft_amd.qc import nlc

B, C = 4.8, 0.0093
CH2 = "C 0 0 0; H 0 0.98934 -0.42079; H 0 -0.98934 -0.42079"


# --------------------------------------------------------------------------- 1. point space
def _cloud():
    """12 points: two coincident (R = 0), one below rho_min, gamma nearly uniform on the first
    half and varying over six decades on the second."""
    rng = np.random.default_rng(7)
    n = 12
    xyz = rng.normal(size=(n, 3)) * 1.5
    xyz[5] = xyz[2]
    w = rng.uniform(0.2, 1.5, n)
    rho = 10.0 ** rng.uniform(-3.0, 0.3, n)
    rho[8] = 3e-9
    gamma = np.empty(n)
    gamma[:6] = 0.3 * (1 + 1e-3 * rng.normal(size=6))
    gamma[6:] = 10.0 ** rng.uniform(-6.0, 0.5, 6)
    return xyz, w, rho, gamma


@pytest.fixture(scope="module")
def cloud_ref():
    import mpmath as mp
    xyz, w, rho, gamma = _cloud()
    active = [i for i in range(len(rho)) if rho[i] > ref.RHO_MIN]
    e = ref.mp_energy(xyz, w, rho, gamma, B, C, active, dps=40)
    grad = ref.mp_gradient(xyz, w, rho, gamma, B, C)
    H, act = ref.mp_hessian(xyz, w, rho, gamma, B, C)
    assert act == active
    return dict(xyz=xyz, w=w, rho=rho, gamma=gamma, active=active, e=e, grad=grad, H=H, mp=mp)


# 40 roundings per term and a sum of at most 48 terms: ~(40 + 48) eps ~ 1e-14; a factor of ten on top
POINT_BOUND = 1e-13


def test_point_space_energy_and_gradient_match_mpmath(cloud_ref):
    r = cloud_ref
    mp = r["mp"]
    g = nlc.ground(r["xyz"], r["w"], r["rho"], r["gamma"], B, C)
    assert abs(mp.mpf(float(g["E"])) - r["e"]) <= POINT_BOUND * abs(r["e"])
    # a gradient entry is a sum of signed pair terms (beta > 0 > F): normalise by the largest
    # entry of its kind, the scale the complex-step and device bounds use too
    for key, col in (("vrho", 0), ("vgamma", 1)):
        scale = max(abs(v) for v in r["grad"][col])
        for i in range(len(r["rho"])):
            err = abs(mp.mpf(float(g[key][i])) - r["grad"][col][i])
            print(key, i, float(err / scale))
            assert err <= POINT_BOUND * scale
    assert g["vrho"][8] == 0.0 and g["vgamma"][8] == 0.0
    vr, vg = ref.first_derivatives(r["xyz"], r["w"], r["rho"], r["gamma"], B, C)
    assert np.max(np.abs(vr - g["vrho"])) <= POINT_BOUND * np.max(np.abs(vr))
    assert np.max(np.abs(vg - g["vgamma"])) <= POINT_BOUND * np.max(np.abs(vg))


def test_point_space_hessian_product_matches_mpmath(cloud_ref):
    r = cloud_ref
    mp = r["mp"]
    n, act = len(r["rho"]), r["active"]
    rng = np.random.default_rng(11)
    x = rng.normal(size=(3, 2, n))          # (vector, rho1 | gamma1, point)
    x[:, 1] *= r["gamma"]                   # gamma1 on gamma's own scale
    vr, vg = ref.hess_apply(r["xyz"], r["w"], r["rho"], r["gamma"], B, C, x[:, 0], x[:, 1])
    m = len(act)
    worst = 0.0
    for v in range(3):
        xv = [mp.mpf(float(x[v, 0, i])) for i in act] + [mp.mpf(float(x[v, 1, i])) for i in act]
        for k in range(2 * m):
            want = sum(r["H"][k, j] * xv[j] for j in range(2 * m))
            norm = sum(abs(r["H"][k, j]) * abs(xv[j]) for j in range(2 * m))
            got = (vr if k < m else vg)[v, act[k % m]]
            err = float(abs(mp.mpf(float(got)) - want) / norm)
            worst = max(worst, err)
            assert err <= POINT_BOUND, (v, k, err)
    print("worst normalised Hessian-product error", worst)
    assert np.all(vr[:, 8] == 0.0) and np.all(vg[:, 8] == 0.0)


# --------------------------------------------------------------------------- 2. AO level
@pytest.fixture(scope="module")
def ch2_ao():
    from xtddft_amd.qc import M
    from xtddft_amd.qc.grid import atomic_grid, becke_partition
    mol = M(CH2, basis="6-31g", charge=0, spin=2)
    xyz, charges = mol.atom_coords(), mol.atom_charges()
    coords, weights, owner = [], [], []
    for ia, z in enumerate(charges):
        c, w, _ = atomic_grid(int(z), 12, 14, prune=False)
        coords.append(c + xyz[ia]); weights.append(w); owner.append(np.full(w.size, ia))
    coords = np.concatenate(coords)
    weights = np.concatenate(weights) * becke_partition(xyz, charges, coords, np.concatenate(owner))
    ao = np.asarray(mol.eval_ao(coords, deriv=1))
    rng = np.random.default_rng(3)
    nao = mol.nao
    # a positive density matrix of 8 electrons' size: 4 random orthonormal-ish orbitals, doubly weighted
    s = mol.intor("int1e_ovlp")
    c = np.linalg.solve(np.linalg.cholesky(s).T, np.linalg.qr(rng.normal(size=(nao, 5)))[0])
    dm0 = 2.0 * c[:, :3] @ c[:, :3].T + c[:, 3:] @ c[:, 3:].T
    rho0, _ = nlc.density(ao, dm0)
    mask = rho0 > nlc.RHO_MIN
    assert 300 <= len(weights) <= 800 and 0 < mask.sum() < len(weights)
    return dict(ao=ao, coords=coords, w=weights, dm0=dm0, mask=mask, nao=nao, rng=rng)


AO_BOUND = 1e-12   # of the largest element: the complex step has no cancellation
H_STEP = 1e-30


def test_ao_potential_is_the_complex_step_derivative_of_the_energy(ch2_ao):
    a = ch2_ao
    e, v = nlc.nlc_vmat(a["ao"], a["coords"], a["w"], a["dm0"], B, C)
    assert np.max(np.abs(v - v.T)) == 0.0
    e_ref = ref.np_energy_ao(a["ao"], a["coords"], a["w"], a["dm0"], B, C, a["mask"])
    assert abs(e - e_ref) <= 1e-13 * abs(e_ref)
    scale = np.max(np.abs(v))
    for _ in range(4):
        x = a["rng"].normal(size=(a["nao"], a["nao"]))
        x = x + x.T
        de = ref.np_energy_ao(a["ao"], a["coords"], a["w"], a["dm0"] + 1j * H_STEP * x, B, C, a["mask"]).imag / H_STEP
        # <V, X> over a direction of unit-size elements: nao^2 terms of size <= scale
        assert abs(np.sum(v * x) - de) <= AO_BOUND * scale * np.sum(np.abs(x))


def test_ao_response_is_the_complex_step_derivative_of_the_potential(ch2_ao):
    a = ch2_ao
    nao = a["nao"]
    d1 = a["rng"].normal(size=(nao, nao))                       # non-symmetric
    r1 = ref.response_ao(a["ao"], a["coords"], a["w"], a["dm0"], d1, B, C)
    _, vc = nlc.nlc_vmat(a["ao"], a["coords"], a["w"], a["dm0"] + 1j * H_STEP * d1, B, C, mask=a["mask"])
    want = vc.imag / H_STEP
    scale = np.max(np.abs(want))
    print("response vs complex step", np.max(np.abs(r1 - want)) / scale)
    assert np.max(np.abs(r1 - want)) <= AO_BOUND * scale
    assert np.max(np.abs(r1 - r1.T)) <= AO_BOUND * scale
    d2 = a["rng"].normal(size=(nao, nao))
    r2 = ref.response_ao(a["ao"], a["coords"], a["w"], a["dm0"], d2, B, C)
    xy, yx = np.sum(d1 * r2), np.sum(d2 * r1)
    # the bilinear form <X, R[Y]>: nao^2 products of elements of size <= |X|max scale
    assert abs(xy - yx) <= AO_BOUND * np.sum(np.abs(d1)) * max(np.max(np.abs(r1)), np.max(np.abs(r2)))


# --------------------------------------------------------------------------- 3. SCF
NLC_GRID = (14, 26)      # per atom, unpruned below 50 angular points: 3 x 364 points


def _ch2_scf(nlc):
    from xtddft_amd.qc import M, ROKS
    mf = ROKS(M(CH2, basis="6-31g", charge=0, spin=2), "b3lyp", nlc=nlc)
    mf.nlc_grid = NLC_GRID
    mf.kernel()
    assert mf.converged
    return mf


@pytest.fixture(scope="module")
def ch2_scf_nlc():
    return _ch2_scf((B, C))


def test_scf_without_nlc_is_the_untouched_branch():
    """nlc=None runs the code path of before: the same bits as a run whose constructor is never
    handed the argument, and no NLC grid is built."""
    from xtddft_amd.qc import M, ROKS
    a = _ch2_scf(None)
    b = ROKS(M(CH2, basis="6-31g", charge=0, spin=2), "b3lyp")
    b.kernel()
    assert a.nlc is None and a.nlc_grids is None and not hasattr(a, "ao_nlc")
    assert a.e_tot == b.e_tot
    assert a.scf_summary == b.scf_summary
    assert np.array_equal(a.mo_energy, b.mo_energy) and np.array_equal(a.mo_coeff, b.mo_coeff)
    mfa = a.to_meanfield()
    assert mfa.nlc is False and mfa.nlc_pars is None and mfa.nlc_grids is None


def test_scf_energy_contains_e_nlc_at_the_converged_density(ch2_scf_nlc):
    mf = ch2_scf_nlc
    plain = _ch2_scf(None)
    dm = mf.make_rdm1()
    g = mf.nlc_grids
    assert g.size == 3 * NLC_GRID[0] * NLC_GRID[1]
    mask = nlc.density(mf.ao_nlc, dm[0] + dm[1])[0] > nlc.RHO_MIN
    e_nlc = ref.np_energy_ao(mf.ao_nlc, g.coords, g.weights, dm[0] + dm[1], B, C, mask)
    # the energy functional of the plain SCF at the NLC density, plus E_nlc
    plain.build()
    e_plain = plain.energy_elec(dm, plain.get_veff(dm=dm))[0] + plain.energy_nuc()
    print("E_nlc", e_nlc, "E_tot", mf.e_tot)
    assert abs(e_nlc) > 1e-3
    assert abs(mf.e_tot - (e_plain + e_nlc)) < 1e-12
    mfield = mf.to_meanfield()
    assert mfield.nlc is True and mfield.nlc_pars == (B, C)
    assert mfield.nlc_grids.ncomp == 4 and mfield.nlc_grids.coords.shape == (g.size, 3)
    # the potential in the converged Fock matrix: veff - plain veff = V_nlc for both spins
    _, v = nlc.nlc_vmat(mf.ao_nlc, g.coords, g.weights, dm[0] + dm[1], B, C)
    dv = mfield.veff - plain.get_veff(dm=dm)[0]
    assert np.abs(dv - v[None]).max() < 1e-12


# --------------------------------------------------------------------------- 4. C ABI
def test_vv10_entries_reject_bad_arguments_without_gpu():
    """Arguments are validated before the first HIP call: XT_ERR_ARG (-1) without a device."""
    from xtddft_amd import _capi
    L = _capi.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(b=B, C=C, rho_min=1e-8)

    def ground(n=4, xyz=p, w=p, rho=p, gam=p, i0=0, i1=4, out=p, **kw):
        q = {**ok, **kw}
        return L.xt_vv10_ground(n, xyz, w, rho, gam, q["b"], q["C"], q["rho_min"], i0, i1, out, None)

    def response(n=4, xyz=p, w=p, rho=p, gam=p, sums=p, nz=2, r1=p, g1=p, i0=0, i1=4, vr=p, vg=p, **kw):
        q = {**ok, **kw}
        return L.xt_vv10_response(n, xyz, w, rho, gam, q["b"], q["C"], q["rho_min"], sums, nz, r1, g1, i0, i1,
                                  vr, vg, None)

    for f in (ground, response):
        assert f(n=-1, i0=0, i1=0) == -1
        assert f(i0=-1) == -1 and f(i0=3, i1=2) == -1 and f(i1=5) == -1
        assert f(b=0.0) == -1 and f(C=-1.0) == -1 and f(rho_min=-1e-9) == -1
        for name in ("xyz", "w", "rho", "gam"):
            assert f(**{name: None}) == -1
        assert b"vv10" in L.xt_last_error()
        assert f(n=0, i0=0, i1=0) == 0 and f(i0=2, i1=2) == 0          # no work: nothing touched
        assert f(i0=2, i1=2, xyz=None, w=None, rho=None, gam=None) == 0
    assert ground(out=None) == -1
    assert response(nz=-1) == -1
    for name in ("sums", "r1", "g1", "vr", "vg"):
        assert response(**{name: None}) == -1
    assert response(nz=0, sums=None, r1=None, g1=None, vr=None, vg=None) == 0
    assert L.xt_set_nlc(None, 4, p, p, p, B, C, 1e-8, _capi.XT_PTR_HOST) == -1
    assert L.xt_abi_version() == 8


def test_vv10_entries_are_declared_everywhere():
    from xtddft_amd import _capi, build
    names = ("xt_set_nlc", "xt_vv10_ground", "xt_vv10_response")
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "xtddft_amd.h")).read()
    for n in names:
        assert n in _capi.EXPORTS and f"int {n}(" in header
    assert "XTDA.py:515-517" in header
    assert "xt_vv10.hip" in build.SOURCES
