"""Host checks of the multicollinear spin-flip TDA gradient on a UKS reference (no GPU):
``mcol.sf_mc_kernel_grad`` against the kernel, the explicit third-derivative tensor and finite
differences; the NumPy restatement ``tests/sfmcgrad_ref.py`` against frozen-grid finite differences of
host energies and against the collinear restatement; the argument checks of the C entries
``xt_xc_resp_sf`` / ``xt_xc_rows``, their export lists, and the refusals of ``SFU_gradient`` /
``SFD_gradient``.  Frozen grid as in ``tests/test_sfksgrad_host.py``."""
import os
import types

import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
import sfksgrad_ref as SK
import sfmcgrad_ref as MC
from xtddft_amd import _capi, build, mcol, qc
from xtddft_amd.grad import SFD_gradient, SFGradients, SFU_gradient
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up

H_FD = 2e-3       # Bohr
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"
GAP = 1e-3        # Ha
SAMPLES = 20
EPS = 2.0 ** -52


def fake_mf(xc):
    """What ``mcol`` reads of a mean field when the densities are given."""
    return types.SimpleNamespace(xc=xc, xctype=qc.xc.xc_type(xc), fxc_sf_mc=None, extra={}, mo_coeff=None, mo_occ=None,
                                 grids=types.SimpleNamespace(ao=None))


# --------------------------------------------------------------------------- sf_mc_kernel_grad
NREG, NTINY, NEMPTY, NOFF = 300, 12, 12, 8


def kernel_inputs(xc):
    """Spin densities (2, nk, G) and a transition density (nk, G): ordinary points, points whose
    densities lie below DENS_THRESHOLD (the kernel is evaluated at RHO_SHIFT there), points with one
    empty spin channel, and points the kernel screens out (RHO_SHIFT keeps the total above the threshold
    for every non-negative density, so these carry a small negative one)."""
    nk = 4 if qc.xc.xc_type(xc) == "GGA" else 1
    rng = np.random.default_rng(11)
    G = NREG + NTINY + NEMPTY + NOFF
    rho = np.zeros((2, nk, G))
    rho[:, 0] = rng.uniform(0.02, 1.0, (2, G))
    if nk == 4:
        rho[:, 1:] = 0.3 * rng.standard_normal((2, 3, G)) * rho[:, :1]
    a, b, c = NREG, NREG + NTINY, NREG + NTINY + NEMPTY
    rho[:, :, a:b] *= 1e-15
    rho[0, :, b:b + NEMPTY // 2] = 0.0
    rho[1, :, b + NEMPTY // 2:c] = 0.0
    rho[:, :, c:] *= 0.0
    rho[:, 0, c:] = -1e-11
    rho1 = 0.1 * rng.standard_normal((nk, G))
    kinds = dict(regular=slice(0, a), tiny=slice(a, b), empty=slice(b, c), off=slice(c, G))
    return rho, rho1, kinds


@pytest.mark.parametrize("xc", ["svwn", "pbe", "b3lyp", "bhandhlyp"])
def test_sf_mc_kernel_grad_against_kernel_tensor_and_differences(xc):
    """12 samples.  q = 2 rho1^T fxc_sf rho1 equals the contraction of ``sf_mc_kernel`` to 1e-13 relative;
    dq equals the contraction of the explicit tensor to 1e-10 of max|dq|, per kind of point (the tiny
    densities have derivatives many orders above the ordinary ones and would hide them); dq = 0 exactly
    at screened points; and for ten directions sum_g v_g dq . u matches Richardson-extrapolated central
    differences of sum_g v_g q: |a - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps / (h/2).  The
    directions are relative steps (u = direction x the point's own density, so no density changes
    sign) on the ordinary points and on the points with one empty spin channel, where they move the
    other channel.  Only the 12 tiny-density points and the 8 screened ones take no step: at a density of
    1e-15 a step of 1e-3 x 1e-15 lies below the rounding of the sum with RHO_SHIFT = 1e-11, so a
    difference quotient there is noise; the tensor covers those points.  q is also held to 1e-13 of the
    largest |q| of each kind of point."""
    mf = fake_mf(xc)
    rho, rho1, kinds = kernel_inputs(xc)
    nk = rho.shape[1]
    q, dq = mcol.sf_mc_kernel_grad(mf, rho1, 12, rho=rho)
    f = mcol.sf_mc_kernel(mf, 12, rho=rho)
    q_ref = 2.0 * np.einsum('xg,xyg,yg->g', rho1, f, rho1)
    s_q = 2.0 * np.einsum('xg,xyg,yg->g', np.abs(rho1), np.abs(f), np.abs(rho1))
    err_q = (np.abs(q - q_ref) / np.maximum(s_q, 1e-300)).max()
    ref = MC.mc_arrays(xc, rho, 12)
    assert np.abs(ref.fsf - f).max() <= 1e-12 * np.abs(f).max()
    dq_ref = 2.0 * np.einsum('xg,xyskg,yg->skg', rho1, ref.kxc, rho1)
    worst = {}
    for kind, sl in kinds.items():
        scale = np.abs(dq_ref[:, :, sl]).max()
        worst[kind] = np.abs(dq[:, :, sl] - dq_ref[:, :, sl]).max() / scale if scale > 0 else 0.0
    print(f"{xc}: max|q - einsum| / S = {err_q:.2e}; max|dq - tensor| / max|dq| per kind {worst}; "
          f"max|dq| regular {np.abs(dq[:, :, kinds['regular']]).max():.3e}")
    assert err_q <= 1e-13
    for kind, sl in kinds.items():             # and relative to the values themselves, per kind of point
        assert np.abs(q[sl] - q_ref[sl]).max() <= 1e-13 * np.abs(q_ref[sl]).max(), kind
    assert np.all(dq[:, :, kinds["off"]] == 0.0) and np.all(q[kinds["off"]] == 0.0)
    assert np.abs(dq[:, :, kinds["regular"]]).max() > 0 and np.abs(dq[:, :, kinds["tiny"]]).max() > 0
    assert max(worst.values()) <= 1e-10
    # finite differences of the contraction of sf_mc_kernel
    rng = np.random.default_rng(5)
    live = np.zeros(rho.shape[2])
    live[kinds["regular"]] = 1.0
    live[kinds["empty"]] = 1.0
    scale = np.abs(rho[:, :1]) * live                          # a relative step of each point's own density
    v = rng.standard_normal(rho.shape[2]) / np.maximum(s_q, 1e-300)             # every point counts alike

    def total(r):
        return float((v * 2.0 * np.einsum('xg,xyg,yg->g', rho1, mcol.sf_mc_kernel(mf, 12, rho=r), rho1)).sum())
    dirs = []
    for s in range(2):
        for k in range(nk):
            u = np.zeros_like(rho)
            u[s, k] = 1.0
            dirs.append(u)
    while len(dirs) < 10:
        dirs.append(rng.standard_normal(rho.shape))
    h = 2e-3
    eps = EPS * float(np.abs(v * s_q).sum())
    for n, u in enumerate(dirs):
        u = u * scale
        a = float((v * (dq * u).sum((0, 1))).sum())
        fine, coarse = R.richardson(lambda s: total(rho + s * u), h)
        lhs, rhs = abs(a - fine), 10 * abs(fine - coarse) + 10 * 2 * eps / (h / 2)
        print(f"  direction {n}: a = {a:+.10e}, FD = {fine:+.10e}, |diff| = {lhs:.2e} <= {rhs:.2e}")
        assert lhs <= rhs


# --------------------------------------------------------------------------- restated gradient
def run_uks(mol, xc, grids, conv_tol=1e-12):
    mf = qc.UKS(mol, xc=xc)
    mf.grids = grids
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
    return min(abs(e[k] - e[j]) for j in (k - 1, k + 1) if 0 <= j < e.size)


@pytest.fixture(scope="module")
def fd_runs():
    """Per functional: the undisplaced UKS and the six displaced ones of one random direction on the same
    coarse frozen grid, each with its XC arrays and its multicollinear kernel (the undisplaced one with
    the third-derivative tensor)."""
    out = {}

    def get(xc):
        if xc not in out:
            mol = qc.M(CH2, basis="6-31g", spin=2)
            grids = K.coarse_grids(mol, 8)
            mf = run_uks(mol, xc, grids)
            ao10 = None
            u = R.random_direction(mol.natm, 1)
            runs = {}
            for s in (2 * H_FD, H_FD, H_FD / 2):
                for sg in (1, -1):
                    m = run_uks(R.displaced(mol, u, sg * s), xc, grids)
                    xa = SK.xc_arrays(m)
                    runs[sg * s] = (m, xa, MC.mc_arrays_of(m, xa, SAMPLES, with_grad=False))
            xa = SK.xc_arrays(mf, ao10)
            out[xc] = (mol, mf, u, runs, R.deriv_eri(mol), xa, MC.mc_arrays_of(mf, xa, SAMPLES), {})
        return out[xc]
    return get


@pytest.mark.parametrize("isf", [-1, 1])
@pytest.mark.parametrize("xc", ["b3lyp", "pbe", "svwn"])
def test_restated_gradient_against_frozen_grid_finite_differences(fd_runs, xc, isf):
    """CH2 / 6-31G on every eighth point of the level-3 grid, frozen; state 1 of the multicollinear
    (20 samples) spin-flip-down and spin-flip-up A matrices, E = e_tot + omega, one random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr.  The root is
    followed by overlap and stays more than 1e-3 Ha from its neighbours at every geometry; the two new
    XC terms each exceed 1e-4 Ha / Bohr."""
    mol, mf, u, runs, ip, xa, mc, mcache = fd_runs(xc)
    state = 0
    e0, xs0 = MC.sf_mc_states(mf, isf, xa, mc)
    assert _separated(e0, state) > GAP, e0[:4]
    g, S, parts = MC.sf_mc_grad(mf, xs0[state], isf, ip, xa, mc, mcache=mcache)
    x0 = _xao(mf, xs0[state], isf)[0]

    def energy(s):
        m, xam, mcm = runs[s]
        e, xs = MC.sf_mc_states(m, isf, xam, mcm)
        k, ov = R.follow(mf.s1e, x0, _xao(m, xs[:6], isf))
        assert ov > 0.9, (s, ov)
        assert _separated(e, k) > GAP, (s, e[:4])
        return m.e_tot + e[k]
    eps_e = max([mf.last_energy_change] + [m[0].last_energy_change for m in runs.values()])
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    e_col = SK.sf_states(mf, isf)[0]
    print(f"SF {isf:+d} state 1, multicollinear, UKS {xc} ({mf.grids.size} points): omega = {e0[state]:.6f} (collinear "
          f"{e_col[state]:.6f}, gap {_separated(e0, state):.2e}), g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, "
          f"|diff| = {lhs:.2e} <= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e}); "
          f"S = {S:.3e}, max|2 G_xc[wv1; X_S]| = {np.abs(parts['xc_sf']).max():.3e}, max|G_xc[wv2; D0]| = "
          f"{np.abs(parts['xc_k']).max():.3e}, sum_A g = {parts['sum_atoms']}")
    assert np.abs(parts["xc_sf"]).max() > 1e-4
    assert np.abs(parts["xc_k"]).max() > 1e-4
    assert lhs <= rhs


@pytest.mark.parametrize("isf", [-1, 1])
def test_restatement_reproduces_the_collinear_one_without_the_kernel(fd_runs, isf):
    """fxc_sf = 0 and kxc_sf = 0: ``sfksgrad_ref.sf_ks_grad`` to 1e-10, and the collinear spectrum."""
    mol, mf, u, runs, ip, xa, mc, _ = fd_runs("b3lyp")
    zero = MC.zero_mc_arrays(xa)
    e_ref, xs = SK.sf_states(mf, isf)
    assert np.abs(MC.sf_mc_states(mf, isf, xa, zero)[0] - e_ref).max() <= 1e-10
    worst = 0.0
    for state in (0, 1):
        ref = SK.sf_ks_grad(mf, xs[state], isf, ip, xa)[0]
        got, _, parts = MC.sf_mc_grad(mf, xs[state], isf, ip, xa, zero)
        assert np.abs(parts["xc_sf"]).max() == 0.0 and np.abs(parts["xc_k"]).max() == 0.0
        worst = max(worst, np.abs(got - ref).max())
    print(f"SF {isf:+d}: max|multicollinear restatement(no kernel) - collinear restatement| = {worst:.2e}")
    assert worst <= 1e-10


# --------------------------------------------------------------------------- the C entries
def test_exports_and_build_lists():
    for name in ("xt_xc_resp_sf", "xt_xc_rows"):
        assert name in _capi.EXPORTS
    assert "xt_xc_resp_sf.hip" in build.SOURCES
    assert _capi.ABI_VERSION == 8                      # pure additions: no bump
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        text = f.read()
    assert "int xt_xc_resp_sf(" in text and "int xt_xc_rows(" in text and "#define XT_ABI_VERSION 8" in text
    assert os.path.exists(os.path.join(root, "xtddft_amd", "csrc", "xt_xc_resp_sf.hip"))
    import xtddft_amd
    assert xtddft_amd.SFU_gradient is SFU_gradient and xtddft_amd.SFD_gradient is SFD_gradient
    assert "SFU_gradient" in xtddft_amd.__all__ and "SFD_gradient" in xtddft_amd.__all__


def _rejected(L, rc, word):
    assert rc == -1, rc
    assert word.encode() in L.xt_last_error(), L.xt_last_error()


def test_xt_xc_resp_sf_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with its own message before the first HIP call; the
    zero-size calls return 0."""
    L = hiplib
    d = np.zeros(256).ctypes.data

    def call(ngrid=2, nao=3, xctype=_capi.XC["GGA"], ao=d, ao_plane=6, ldao=3, c=d, ldc=3, fxc=d, ldg=2, w=d,
             rho1=d, wv=d, ldo=2, b=d, ldb=3):
        return L.xt_xc_resp_sf(ngrid, nao, xctype, ao, ao_plane, ldao, c, ldc, fxc, ldg, w, rho1, wv, ldo, b, ldb, None)
    for name in ("ngrid", "nao", "ao_plane", "ldao", "ldc", "ldg", "ldo", "ldb"):
        _rejected(L, call(**{name: -1}), "negative size")
    for flag in (_capi.XC["HF"], _capi.XC["MGGA"], 7):
        _rejected(L, call(xctype=flag), "xctype")
    for name in ("ldao", "ldc", "ldb"):
        _rejected(L, call(**{name: 2}), name)
        _rejected(L, call(**{name: 2}, xctype=_capi.XC["LDA"]), name)
    _rejected(L, call(ldg=1), "ldg")
    _rejected(L, call(ldo=1), "ldo")
    _rejected(L, call(ao_plane=5), "ao_plane")
    assert call(ao_plane=0, xctype=_capi.XC["LDA"], ao=None) == -1 and b"null" in L.xt_last_error()
    _rejected(L, call(ngrid=2**40, ldg=2**40, ldo=2**40, ao_plane=2**44), "blocks")
    for name in ("ao", "c", "fxc", "w"):
        _rejected(L, call(**{name: None}), "null")
        _rejected(L, call(**{name: None}, xctype=_capi.XC["LDA"]), "null")
    assert call(ngrid=0, ao=None, c=None, fxc=None, w=None, ldg=0, ldo=0, ao_plane=0) == 0
    assert call(nao=0, ao=None, c=None, fxc=None, w=None) == 0
    assert call(rho1=None, wv=None, b=None, ao=None) == 0


def test_xt_xc_rows_rejects_bad_arguments_without_gpu(hiplib):
    L = hiplib
    d = np.zeros(256).ctypes.data

    def call(ngrid=2, nao=3, xctype=_capi.XC["GGA"], nch=2, ao=d, ao_plane=6, ldao=3, wv=d, ldo=2, b=d, ldb=3):
        return L.xt_xc_rows(ngrid, nao, xctype, nch, ao, ao_plane, ldao, wv, ldo, b, ldb, None)
    for name in ("ngrid", "nao", "ao_plane", "ldao", "ldo", "ldb"):
        _rejected(L, call(**{name: -1}), "negative size")
    for flag in (_capi.XC["HF"], _capi.XC["MGGA"], 7):
        _rejected(L, call(xctype=flag), "xctype")
    for nch in (0, 5, -1):
        _rejected(L, call(nch=nch), "nch")
    for name in ("ldao", "ldb"):
        _rejected(L, call(**{name: 2}), name)
        _rejected(L, call(**{name: 2}, xctype=_capi.XC["LDA"]), name)
    _rejected(L, call(ldo=1), "ldo")
    _rejected(L, call(ao_plane=5), "ao_plane")
    _rejected(L, call(ngrid=2**40, ldo=2**40, ao_plane=2**44), "blocks")
    for name in ("ao", "wv"):
        _rejected(L, call(**{name: None}), "null")
        _rejected(L, call(**{name: None}, xctype=_capi.XC["LDA"]), "null")
    assert call(ngrid=0, ao=None, wv=None, ldo=0, ao_plane=0) == 0
    assert call(nao=0, ao=None, wv=None) == 0
    assert call(b=None, ao=None, wv=None) == 0


# --------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def host_scfs():
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, 8)

    def make(build_mf, device=True):
        mf = build_mf(mol)
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
    down, up = SF_TDA_down(mfield, method=1, davidson=False), SF_TDA_up(mfield, method=1, davidson=False)
    # accepted, with the reference's attributes and the sample count of the solver path
    for cls, td in ((SFD_gradient, down), (SFU_gradient, up)):
        gm = cls(td)
        assert isinstance(gm, SFGradients) and gm.is_ks
        assert (gm.method, gm.state, gm.cphf_conv_tol, gm.cphf_max_cycle, gm.atmlst, gm.de) == (1, 1, 1e-10, 500, None, None)
        assert gm.collinear_samples == 30 and gm.timings == {} and gm.de_xc is None
        assert cls(td, method=1, state=3).state == 3
        with pytest.raises(RuntimeError):                                  # the TDA kernel() has not run
            gm.kernel()
    assert SFD_gradient(SF_TDA_down(mfield, method=1, davidson=True)).collinear_samples == 50
    assert SFD_gradient(SF_TDA_down(mfield, method=1, davidson=True, collinear_samples=24)).collinear_samples == 24
    assert SFD_gradient(SF_TDA_down(mfield, method=2, davidson=False), method=2).collinear_samples is None
    # the wrong TDA class, a method that is not the one of the roots, method 0
    with pytest.raises(TypeError):
        SFU_gradient(down)
    with pytest.raises(TypeError):
        SFD_gradient(up)
    with pytest.raises(TypeError):
        SFD_gradient(mfield)
    with pytest.raises(ValueError):
        SFD_gradient(down, method=2)
    with pytest.raises(ValueError):
        SFU_gradient(SF_TDA_up(mfield, method=2, davidson=False))          # the default is method = 1
    with pytest.raises(NotImplementedError):
        SFD_gradient(SF_TDA_down(mfield, method=0, davidson=False), method=0)
    # nuc_grad_method() still refuses the multicollinear kernel and names the way in
    with pytest.raises(NotImplementedError) as err:
        down.nuc_grad_method()
    assert "multicollinear" in str(err.value) and "SFU_gradient" in str(err.value) and "SFD_gradient" in str(err.value)
    # a KS mean field on the host
    host, hfield = make(lambda m: qc.UKS(m, xc="b3lyp"), device=False)
    with pytest.raises(NotImplementedError) as err:
        SFD_gradient(SF_TDA_down(hfield, method=1, davidson=False))
    assert "host" in str(err.value)
    # everything check_ks_gradient_mf refuses
    for build_mf in (lambda m: qc.ROKS(m, xc="b3lyp"), lambda m: qc.UKS(m, xc="tpss"),
                     lambda m: qc.UKS(m, xc="cam-b3lyp"), lambda m: qc.UKS(m, xc="b3lyp", nlc=(6.0, 0.01)),
                     lambda m: qc.UKS(m, xc="b3lyp").density_fit(), lambda m: qc.UKS(m, xc="b3lyp").sfx2c1e()):
        keep, field = make(build_mf)
        with pytest.raises(NotImplementedError):
            SFD_gradient(SF_TDA_down(field, method=1, davidson=False))
    # a Hartree-Fock reference has no multicollinear kernel
    hf, hffield = make(lambda m: qc.UHF(m))
    with pytest.raises(NotImplementedError):
        SFD_gradient(SF_TDA_down(hffield, method=1, davidson=False))
