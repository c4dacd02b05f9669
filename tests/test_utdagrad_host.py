"""Host checks of the U-TDA gradient (no GPU): the argument checks and export lists of the C entry
``xt_grad_jk2``, the amplitude mapping of ``grad_utda.utda_amplitudes``, the third-derivative weights
of ``qc.xc.kernel_grad_torch`` against the contraction of ``eval_xc_eff_torch`` and its central
differences, the NumPy restatement ``tests/utdagrad_ref.py`` against finite differences of its own
E_SCF + omega on a grid frozen in space, and the refusals of the driver.

Frozen grid: every displaced SCF gets the undisplaced ``Grids`` object, as in
``tests/test_sfksgrad_host.py``; translational invariance does not hold on such a grid."""
import os

import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
import sfksgrad_ref as SK
import utdagrad_ref as U
from xtddft_amd import _capi, qc
from xtddft_amd.utils import order_pyscf2my
from xtddft_amd.xtda import XTDA

H_FD = 2e-3       # Bohr
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # the bent geometry of tests/test_gpu_grad.py (Angstrom)
GAP = 1e-3        # Ha: the root is separated from its neighbours by more than this


# --------------------------------------------------------------------------- the C entry
def test_exports_and_header():
    assert "xt_grad_jk2" in _capi.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        text = f.read()
    assert "int xt_grad_jk2(" in text and "int xt_grad_jk(" in text
    from xtddft_amd.qc import grad as G
    assert callable(G.grad_jk_lists) and G.MAX_TERMS == 8


def test_xt_grad_jk2_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with a message that names the argument, before the
    first HIP call; the zero-size calls return 0; an empty list may be null."""
    L = hiplib
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data

    def call(nbra=1, binfo=i, bprim=d, eb=d, bao=i, nket=1, kinfo=i, kprim=d, ek=d, kao=i, lbra=3, lket=2, nj=2,
             wj=d, pj=d, qj=d, nk=2, wk=d, pk=d, qk=d, nao=1, strip=1, natm=1, work=d, nwork=6, out=d):
        return L.xt_grad_jk2(nbra, binfo, bprim, eb, bao, nket, kinfo, kprim, ek, kao, lbra, lket, nj, wj, pj, qj,
                             nk, wk, pk, qk, nao, strip, natm, work, nwork, out, None)

    def rejected(rc, *words):
        assert rc == -1, rc
        msg = L.xt_last_error()
        assert b"xt_grad_jk2" in msg, msg
        for word in words:
            assert word.encode() in msg, msg
    for name in ("nbra", "nket", "nao", "natm", "nwork"):
        rejected(call(**{name: -1}), "negative size")
    rejected(call(strip=0), "strip")
    for lb, lk in ((-1, 2), (3, -1), (9, 0), (8, 7), (7, 8)):
        rejected(call(lbra=lb, lket=lk), "order")
    for bad in (-1, 9):
        rejected(call(nj=bad), "nj")
        rejected(call(nk=bad), "nk")
    rejected(call(nj=0, nk=0), "both zero")
    rejected(call(nj=0, nk=0, wj=None, pj=None, qj=None, wk=None, pk=None, qk=None), "both zero")
    rejected(call(wj=None), "null", "wj")
    rejected(call(wk=None), "null", "wk")
    for name in ("pj", "qj"):
        rejected(call(**{name: None}), "null", "pj or qj")
    for name in ("pk", "qk"):
        rejected(call(**{name: None}), "null", "pk or qk")
    for name in ("binfo", "bprim", "eb", "bao", "kinfo", "kprim", "ek", "kao", "work", "out"):
        rejected(call(**{name: None}), "null")
    rejected(call(nwork=5), "workspace")
    rejected(call(nket=5, strip=2, nwork=11), "workspace")        # 3 strips + 1: 12 doubles
    rejected(call(nket=5, strip=2**31 - 1, nwork=5), "workspace")  # no int overflow in the strip count
    # an empty list is not read: with the other list complete its pointers may be null, and the checks
    # that follow are reached
    rejected(call(nj=0, wj=None, pj=None, qj=None, nwork=5), "workspace")
    rejected(call(nk=0, wk=None, pk=None, qk=None, nwork=5), "workspace")
    assert call(nbra=0, binfo=None, out=None) == 0 and call(nket=0, kinfo=None) == 0      # nothing to add
    assert call(nbra=0, nk=0, wk=None, pk=None, qk=None) == 0
    assert call(natm=0, nj=0, wj=None, pj=None, qj=None, out=None) == 0


# --------------------------------------------------------------------------- amplitudes
def test_amplitude_mapping_reproduces_the_transition_moments():
    """X_a, X_b from a seeded ``td.v`` give the moments of ``td._transition`` for every root, and their
    norm is 1."""
    from xtddft_amd.grad_utda import utda_amplitudes
    mol = qc.M(CH2, basis="6-31g", spin=2)
    mf = R.run_uhf(mol, conv_tol=1e-9)
    mfield = mf.to_meanfield()
    td = XTDA(mol, mfield, nstates=3, use_Davidson=False)
    info = mfield.shape_info()
    td.nc, td.no, td.nv = info['nc'], info['no'], info['nv']
    td.order = order_pyscf2my(td.nc, td.no, td.nv)
    dim = (td.nc + td.no) * td.nv + td.nc * (td.no + td.nv)
    rng = np.random.default_rng(11)
    td.v = rng.standard_normal((dim, 3))
    td._split_blocks()
    dip = rng.standard_normal((3, mol.nao, mol.nao))
    dip = dip + dip.transpose(0, 2, 1)
    want = td._transition(dip)
    coa, cva, cob, cvb = td._spin_orbitals()
    for r in range(3):
        xa, xb = utda_amplitudes(td, r)
        assert xa.shape == (cva.shape[1], coa.shape[1]) and xb.shape == (cvb.shape[1], cob.shape[1])
        assert abs(np.sum(xa * xa) + np.sum(xb * xb) - 1.0) <= 1e-14
        got = (np.einsum('xpq,pi,qa,ai->x', dip, coa, cva, xa) + np.einsum('xpq,pi,qa,ai->x', dip, cob, cvb, xb))
        got = got * np.linalg.norm(td.v[:, r])
        assert np.abs(got - want[r]).max() <= 1e-12 * np.abs(want[r]).max()


# --------------------------------------------------------------------------- third-derivative weights
def density_table(ncomp, seed=5):
    """(rho0, rho1) (2, ncomp, 200): total densities spread over 1e-6 .. 1 with a spin polarisation of at
    most 0.9 (two channels six decades apart would make every derivative with respect to the small one
    a rounding error of q, which no difference quotient resolves) and gradients of reduced size O(1); points 0..9 below DENS_THRESHOLD in rho_a + rho_b, points 10..19 just above it, points
    20..29 with a vanishing beta channel.  rho1 of a channel scales with that channel's own density, as
    the response density of an orbital product does."""
    from xtddft_amd.qc import xc as X
    rng = np.random.default_rng(seed)
    G = 200
    r0 = np.zeros((2, ncomp, G))
    u = rng.uniform(-6, 0, (2, G))
    tot, zeta = 10.0 ** u[0], 0.9 * (u[1] / 3.0 + 1.0)             # rho_a + rho_b over 1e-6 .. 1, |zeta| <= 0.9
    r0[0, 0], r0[1, 0] = 0.5 * tot * (1.0 + zeta), 0.5 * tot * (1.0 - zeta)
    r0[:, 0, :10] = X.DENS_THRESHOLD * 10.0 ** rng.uniform(-2, -0.5, (2, 10))
    r0[:, 0, 10:20] = X.DENS_THRESHOLD * 10.0 ** rng.uniform(0.5, 2, (2, 10))
    r0[1, 0, 20:30] = 0.0
    if ncomp > 1:
        r0[:, 1:] = rng.standard_normal((2, ncomp - 1, G)) * (r0[:, 0] ** (4.0 / 3.0))[:, None]
    r1 = rng.standard_normal((2, ncomp, G)) * r0[:, :1]
    if ncomp > 1:
        r1[:, 1:] *= (r0[:, :1] ** (1.0 / 3.0))
    return r0, r1


@pytest.mark.parametrize("xc", ["svwn", "pbe", "b3lyp"])
def test_third_derivative_weights(xc):
    """q against the contraction rho1^T fxc rho1 of ``eval_xc_eff_torch`` to 1e-13, dq against central
    differences of that contraction (relative step 1e-4) to 1e-5, both elementwise in
    |a - b| / (|a| + |b|), nothing subtracted.
    Screened points give exact zeros.  Where the beta channel vanishes the contraction switches its
    exchange half off at the point itself, so a central difference across it means nothing: there the
    alpha components are compared and the beta ones must be finite."""
    import torch
    from xtddft_amd.qc import xc as X
    nc = X.NCOMP[X.xc_type(xc)]
    r0, r1 = density_table(nc)
    t1 = torch.as_tensor(r1)

    def contraction(r):
        f = X.eval_xc_eff_torch(xc, torch.as_tensor(r), deriv=2)[2]
        return torch.einsum('skg,sktlg,tlg->g', t1, f, t1).numpy()
    q, dq = X.kernel_grad_torch(xc, torch.as_tensor(r0), t1)
    q, dq = q.numpy(), dq.numpy()
    assert dq.shape == r0.shape and np.isfinite(q).all() and np.isfinite(dq).all()
    ref = contraction(r0)
    screened = (r0[0, 0] + r0[1, 0]) <= X.DENS_THRESHOLD
    assert screened.sum() == 10
    assert np.all(q[screened] == 0.0) and np.all(dq[:, :, screened] == 0.0) and np.all(ref[screened] == 0.0)
    den = np.abs(q) + np.abs(ref)
    rel_q = np.where(den > 0, np.abs(q - ref) / np.where(den > 0, den, 1.0), 0.0)
    live = ~screened
    assert np.abs(q[live]).min() > 0
    worst = 0.0
    n_all = 0
    for s in range(2):
        for k in range(nc):
            scale = np.abs(r0[s, k]) if k == 0 else np.maximum(np.abs(r0[s, k]), r0[s, 0] ** (4.0 / 3.0))
            step = 1e-4 * scale
            ok = live & (step > 0)
            hp, hm = r0.copy(), r0.copy()
            hp[s, k] += step
            hm[s, k] -= step
            fd = np.zeros_like(q)
            fd[ok] = (contraction(hp)[ok] - contraction(hm)[ok]) / (2 * step[ok])
            a, b = dq[s, k][ok], fd[ok]
            err = np.abs(a - b) / np.maximum(np.abs(a) + np.abs(b), 1e-300)
            worst = max(worst, float(err.max()))
            n_all += a.size
            if s == 1:
                assert not ok[20:30].any()          # vanishing beta: no difference quotient
            else:
                assert ok[20:30].all()
    print(f"{xc}: max rel |q - contraction| = {rel_q.max():.2e}, max rel |dq - central difference| = {worst:.2e} "
          f"over {n_all} elements")
    assert rel_q.max() <= 1e-13
    assert worst <= 1e-5


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


def _separated(e, k):
    return min(abs(e[k] - e[j]) for j in (k - 1, k + 1) if 0 <= j < e.size)


@pytest.mark.parametrize("xc", ["hf", "b3lyp"])
def test_restated_gradient_against_frozen_grid_finite_differences(xc):
    """CH2 triplet / 6-31G, Hartree-Fock and B3LYP (every eighth point of the level-3 grid, frozen);
    state 1 of the dense U-TDA A matrix, E = e_tot + omega, one random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr.
    The root is followed by the overlap of the AO transition densities and stays more than 1e-3 Ha from
    its neighbours; with the functional, the part the third derivative adds must exceed 1e-4 Ha / Bohr."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    ks = xc != "hf"
    grids = K.coarse_grids(mol, 8) if ks else None

    def run(m):
        return run_uks(m, xc, grids) if ks else R.run_uhf(m)

    def arrays(m):
        return SK.xc_arrays(m) if ks else SK.zero_xc_arrays(m.mol.nao)
    mf = run(mol)
    xa = arrays(mf)
    kxc = U.kxc_arrays(mf, xa) if ks else U.zero_kxc()
    state = 0
    e0, xs0 = U.utda_states(mf, xa)
    assert _separated(e0, state) > GAP, e0[:4]
    g, S, parts = U.utda_grad(mf, xs0[state], R.deriv_eri(mol), xa, kxc)
    assert abs(parts["omega"] - e0[state]) <= 1e-9       # the functional is the eigenvalue
    u = R.random_direction(mol.natm, 1)
    x0 = U.xao(mf, xs0[state])
    eps = [mf.last_energy_change]

    def energy(s):
        m = run(R.displaced(mol, u, s))
        assert not ks or m.grids is grids
        eps.append(m.last_energy_change)
        e, xs = U.utda_states(m, arrays(m))
        k, ov = U.follow(mf.s1e, x0, [U.xao(m, x) for x in xs[:6]])
        assert ov > 0.9, (s, ov)
        assert _separated(e, k) > GAP, (s, e[:4])
        return m.e_tot + e[k]
    fine, coarse = R.richardson(energy, H_FD)
    eps_e = max(abs(v) for v in eps)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    kpart = float(np.abs(parts["xc_kxc"]).max())
    print(f"U-TDA state 1 on {xc}: omega = {e0[state]:.6f}, g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, "
          f"|diff| = {lhs:.2e} <= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e}); "
          f"S = {S:.3e}, max|third-derivative part| = {kpart:.3e}, sum_A g = {parts['sum_atoms']}")
    if ks:
        assert kpart > 1e-4
    else:
        assert np.abs(parts["sum_atoms"]).max() <= 1e-9
    assert lhs <= rhs


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
    from xtddft_amd.grad_utda import UTDAGradients
    mol, make = host_scfs
    # ROKS: X-TDA
    ro, rofield = make(lambda m: qc.ROKS(m, xc="b3lyp"))
    with pytest.raises(NotImplementedError) as err:
        XTDA(mol, rofield, use_Davidson=False).nuc_grad_method()
    assert "xtdhf.py" in str(err.value) and "variational" in str(err.value)
    uks, mfield = make(lambda m: qc.UKS(m, xc="b3lyp"))
    with pytest.raises(NotImplementedError) as err:
        XTDA(mol, mfield, basis='tensor', use_Davidson=False).nuc_grad_method()
    assert "tensor" in str(err.value)
    # a KS mean field on the host
    host, hfield = make(lambda m: qc.UKS(m, xc="b3lyp"), device=False)
    with pytest.raises(NotImplementedError) as err:
        XTDA(mol, hfield, use_Davidson=False).nuc_grad_method()
    assert "host" in str(err.value)
    # everything check_ks_gradient_mf refuses
    for build_mf in (lambda m: qc.UKS(m, xc="tpss"), lambda m: qc.UKS(m, xc="cam-b3lyp"),
                     lambda m: qc.UKS(m, xc="b3lyp", nlc=(6.0, 0.01)),
                     lambda m: qc.UKS(m, xc="b3lyp").density_fit(), lambda m: qc.UKS(m, xc="b3lyp").sfx2c1e()):
        keep, field = make(build_mf)
        with pytest.raises(NotImplementedError):
            XTDA(mol, field, use_Davidson=False).nuc_grad_method()
    # ... and check_gradient_mf on Hartree-Fock
    for build_mf in (lambda m: qc.UHF(m).density_fit(), lambda m: qc.UHF(m).sfx2c1e()):
        keep, field = make(build_mf)
        with pytest.raises(NotImplementedError):
            XTDA(mol, field, use_Davidson=False).nuc_grad_method()
    # accepted: the interface of SFGradients
    td = XTDA(mol, mfield, nstates=3, use_Davidson=False)
    gm = td.nuc_grad_method()
    assert isinstance(gm, UTDAGradients) and gm.is_ks
    assert (gm.state, gm.cphf_conv_tol, gm.cphf_max_cycle, gm.atmlst, gm.xc_chunk, gm.de) == (1, 1e-10, 500, None, None, None)
    assert gm.timings == {}
    with pytest.raises(ValueError):                     # the XTDA kernel() has not run
        gm.kernel()
    # a seeded solution: the state checks come before any device work
    info = mfield.shape_info()
    td.nc, td.no, td.nv = info['nc'], info['no'], info['nv']
    td.order = order_pyscf2my(td.nc, td.no, td.nv)
    dim = (td.nc + td.no) * td.nv + td.nc * (td.no + td.nv)
    td.v = np.linalg.qr(np.random.default_rng(3).standard_normal((dim, 3)))[0]
    for state in (0, 4, -1):
        with pytest.raises(ValueError):
            gm.kernel(state=state)
    td.use_Davidson, td.converged = True, np.array([True, False, True])
    with pytest.raises(RuntimeError) as err:
        gm.kernel(state=2)
    assert "not converged" in str(err.value)
    hf, hffield = make(lambda m: qc.UHF(m))
    assert not XTDA(mol, hffield, use_Davidson=False).nuc_grad_method().is_ks
