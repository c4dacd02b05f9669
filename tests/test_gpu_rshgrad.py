"""GPU: nuclear gradients of the range-separated hybrids (CAM-B3LYP, wB97X-D) through the ``.Gradients()``
doors -- the UKS ground state, spin-flip TDA states (collinear and multicollinear) and U-TDA states --
on CH2 triplet.  Their exchange is hyb K + (alpha - hyb) K_LR; the long-range part of the two-electron
derivative term runs through ``xt_grad_jk2_lr`` (``qc.grad.grad_jk_rsh``).

* ground state, CH2 / cc-pVDZ (24 AOs, d shells), both functionals: against the restatement
  ``rsh_ref.uks_grad_rsh`` to 1e-9, the bound of ``test_uks_gradient_on_device_against_restatement``;
* the long-range call alone: ``grad_jk_lists(..., omega=...)`` against ``grad_ref.gamma_contract`` on the dense
  long-range derivative ERIs with random non-symmetric P and Q, inside 1e-12 of the summed magnitudes;
* excited states, CH2 / 6-31G: against finite differences of the device's own E_SCF + omega on a grid frozen
  in space, the state followed by overlap, with the rule of the other gradient tests,
      |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2),  h = 2e-3 Bohr.
  A long-range term missing from the coupling, the right-hand side, the response, W or the kernel lists
  shifts g.u by far more than that.  Every excited-state gradient also runs the driver's own check that the
  omega of its coupling reproduces the TDA root to 1e-9 Ha (``grad.check_root``).

The 6-31G cases run on every fourth point of the level-3 grid (``ksgrad_ref.coarse_grids``), as
tests/test_gpu_utdagrad.py does: the gradient is the exact derivative on whatever fixed grid the mean
field carries."""
import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
import rsh_ref
import utdagrad_ref as UR
from xtddft_amd import grad as SFG
from xtddft_amd import qc
from xtddft_amd.grad import SFGradients, sf_amplitude
from xtddft_amd.grad_utda import UTDAGradients, utda_amplitudes
from xtddft_amd.qc import grad as G
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up
from xtddft_amd.xtda import XTDA

pytestmark = pytest.mark.gpu

H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)
STRIDE = 4
STEPS = tuple(sg * s for s in (2 * H_FD, H_FD, H_FD / 2) for sg in (1, -1))


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _device_uks(mol, xc, grids=None):
    mf = qc.UKS(mol, xc=xc)
    if grids is not None:
        mf.grids = grids             # build() keeps a grid that is already set
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


# --------------------------------------------------------------------------- ground state, cc-pVDZ
@pytest.fixture(scope="module")
def ch2_dz(torch):
    mol = qc.M(CH2, basis="cc-pvdz", spin=2)
    assert mol.nao == 24
    return dict(mol=mol, ip=R.deriv_eri(mol), ip_lr={}, grids=None)


@pytest.mark.parametrize("xc", ["cam-b3lyp", "wb97xd"])
def test_ground_state_against_restatement(ch2_dz, xc):
    w = ch2_dz
    mol = w["mol"]
    mf = _device_uks(mol, xc, w["grids"])
    w["grids"] = mf.grids
    assert mf.omega > 0 and mf.alpha != mf.hyb
    if mf.omega not in w["ip_lr"]:
        w["ip_lr"][mf.omega] = rsh_ref.deriv_eri_lr(mol, mf.omega)
    gm = mf.Gradients()
    assert isinstance(gm, G.KSGradients)
    g = gm.kernel()
    ref = rsh_ref.uks_grad_rsh(mf, w["ip"], w["ip_lr"][mf.omega])
    no_lr = K.uks_grad(mf, w["ip"])[0]
    print(f"UKS {xc} CH2 / cc-pVDZ: omega {mf.omega}, hyb {mf.hyb}, alpha {mf.alpha}; max|g| = {np.abs(ref).max():.4e}, "
          f"max|long-range part| = {np.abs(ref - no_lr).max():.3e}, max|device - restatement| = {np.abs(g - ref).max():.2e}; "
          f"full-range call {gm.timings['grad_jk_full_s']:.4f} s, long-range call {gm.timings['grad_jk_lr_s']:.4f} s")
    assert g.shape == (3, 3) and len(gm.timings["buckets_lr"]) == len(gm.timings["buckets"]) > 0
    assert max(b["bra_order"] for b in gm.timings["buckets_lr"]) >= 5      # the d bucket ran under attenuation
    assert np.abs(ref - no_lr).max() > 1e-4            # the long-range term is a real part of what is checked
    assert np.abs(g - ref).max() <= 1e-9
    assert np.abs(g[:, 0]).max() <= 1e-10              # out of the molecular plane
    assert mf.Gradients().kernel(atmlst=[2]).tobytes() == g[2:3].tobytes()
    with pytest.raises(NotImplementedError, match=r"Gradients\(\)"):
        mf.nuc_grad_method()


@pytest.mark.parametrize("omega", [0.33, 0.2])
def test_long_range_call_alone_against_dense_contraction(torch, omega):
    """s, p and d shells on three centres, three Coulomb and three exchange pairs of random non-symmetric
    matrices through ``grad_jk_lists(..., omega=omega)``; and the two calls of ``grad_jk_rsh``."""
    mol = R.shell_set("spd")
    rng = np.random.default_rng(17)
    n = mol.nao
    jl = [(float(rng.choice([1.0, -0.5, 2.0])), rng.standard_normal((n, n)), rng.standard_normal((n, n))) for _ in range(3)]
    kl = [(float(rng.choice([-1.0, 0.5, -2.0])), rng.standard_normal((n, n)), rng.standard_normal((n, n))) for _ in range(3)]
    ip, ip_lr = R.deriv_eri(mol), rsh_ref.deriv_eri_lr(mol, omega)
    terms = [(w, 0.0, p, q) for w, p, q in jl] + [(0.0, w, p, q) for w, p, q in kl]
    ref, mag = R.gamma_contract(mol, ip_lr, terms, parts=True)
    got = G.grad_jk_lists(mol, jl, kl, 0, omega=omega)
    full = G.grad_jk_lists(mol, jl, kl, 0)
    print(f"omega {omega}: max|g_lr| = {np.abs(ref).max():.3e}, summed magnitudes {mag:.3e}, |device - dense| = "
          f"{np.abs(got - ref).max():.2e}; max|g_lr - g_full| = {np.abs(got - full).max():.3e}")
    assert np.abs(got - full).max() > 1e-3 * np.abs(full).max()
    assert np.abs(got - ref).max() <= 1e-12 * mag
    assert G.grad_jk_lists(mol, jl, kl, 0, omega=omega).tobytes() == got.tobytes()
    assert G.grad_jk_lists(mol, jl, kl, 0, omega=0.0).tobytes() == full.tobytes()
    # hyb K + (alpha - hyb) K_LR as the drivers send it
    hyb, alpha = rsh_ref.CAM_HYB, rsh_ref.CAM_ALPHA
    st = {}
    two = G.grad_jk_rsh(mol, jl, kl, omega, hyb, alpha, 0, stats=st)
    r_full, m_full = R.gamma_contract(mol, ip, [(w, 0.0, p, q) for w, p, q in jl] + [(0.0, hyb * w, p, q) for w, p, q in kl],
                                      parts=True)
    r_lr, m_lr = R.gamma_contract(mol, ip_lr, [(0.0, (alpha - hyb) * w, p, q) for w, p, q in kl], parts=True)
    assert np.abs(two - (r_full + r_lr)).max() <= 1e-12 * (m_full + m_lr)
    assert len(st["buckets"]) == len(st["buckets_lr"]) > 0 and st["full_s"] > 0 and st["lr_s"] > 0
    # hyb = 0: the long-range call runs alone for the exchange; the Coulomb list still goes to call 1
    st = {}
    lone = G.grad_jk_rsh(mol, [], kl, omega, 0.0, 1.0, 0, stats=st)
    assert "buckets" not in st and len(st["buckets_lr"]) > 0
    r_k, m_k = R.gamma_contract(mol, ip_lr, [(0.0, w, p, q) for w, p, q in kl], parts=True)
    assert np.abs(lone - r_k).max() <= 1e-12 * m_k


# --------------------------------------------------------------------------- excited states, 6-31G
@pytest.fixture(scope="module")
def world(torch):
    """Per functional: CH2 / 6-31G on the coarse frozen grid, the device mean field and, on first use, the six
    displaced mean fields of the finite differences (one seeded direction, shared by every driver)."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, STRIDE)
    u = R.random_direction(mol.natm, 3)
    cache = {}

    def case(xc):
        if xc not in cache:
            cache[xc] = dict(mol=mol, u=u, mf=_device_uks(mol, xc, grids), fd=None)
        c = cache[xc]
        if c["fd"] is None:
            c["fd"] = {s: _device_uks(R.displaced(mol, u, s), xc, grids) for s in STEPS}
            assert all(m.grids is grids for m in c["fd"].values())
        return c
    return case


def _sf(isf, method):
    """(make the dense states of a mean field, AO transition density of a root, follow a root)."""
    def make(mf):
        td = (SF_TDA_down if isf == -1 else SF_TDA_up)(mf.to_meanfield(), method=method, davidson=False)
        td.kernel(nstates=2)
        return td

    def xao(mf, td, root):
        s = (0, 1) if isf == -1 else (1, 0)
        co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
        cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
        return cv @ sf_amplitude(td, root) @ co.T
    return make, xao, lambda s1e, x0, xs: R.follow(s1e, x0, np.asarray(xs))


def _utda():
    def make(mf):
        td = XTDA(mf.mol, mf.to_meanfield(), nstates=6, use_Davidson=False)
        td.kernel()
        return td

    def xao(mf, td, root):
        return UR.xao(mf, utda_amplitudes(td, root))
    return make, xao, UR.follow


DRIVERS = {
    "sf_down_2": (_sf(-1, 2), SFGradients),
    "sf_up_2": (_sf(1, 2), SFGradients),
    "sf_down_1": (_sf(-1, 1), SFG.SFD_gradient),      # the multicollinear kernel at its default sample count
    "utda": (_utda(), UTDAGradients),
}


def _fd_rule(what, g, u, energy, eps_e):
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"{what}: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= {rhs:.2e} "
          f"(Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs


def _eps(c):
    return max([abs(c["mf"].last_energy_change)] + [abs(m.last_energy_change) for m in c["fd"].values()])


def test_ground_state_against_finite_differences(world):
    c = world("cam-b3lyp")
    g = c["mf"].Gradients().kernel()
    _fd_rule("UKS cam-b3lyp", g, c["u"], lambda s: c["fd"][s].e_tot, _eps(c))


@pytest.mark.parametrize("xc,driver", [("cam-b3lyp", "sf_down_2"), ("cam-b3lyp", "sf_up_2"), ("cam-b3lyp", "sf_down_1"),
                                       ("cam-b3lyp", "utda"), ("wb97xd", "sf_down_2"), ("wb97xd", "utda")])
def test_excited_state_against_finite_differences(world, xc, driver):
    """State 1 through ``td.Gradients(state=1)``; wB97X-D has alpha = 1, so k_lr = 1 - hyb."""
    c = world(xc)
    mf, u = c["mf"], c["u"]
    (make, xao, follow), cls = DRIVERS[driver]
    td = make(mf)
    with pytest.raises(NotImplementedError):
        td.nuc_grad_method()
    gm = td.Gradients(state=1)
    assert type(gm) is cls and gm.state == 1
    g = gm.kernel()                  # runs grad.check_root: the coupling's omega against td.e[0] to 1e-9 Ha
    tm = gm.timings
    assert tm["zvector_residual"] <= 1e-10 and len(tm["buckets_lr"]) == len(tm["buckets"]) > 0
    x0 = xao(mf, td, 0)

    def energy(s):
        m = c["fd"][s]
        t = make(m)
        k, ov = follow(mf.s1e, x0, [xao(m, t, r) for r in range(6)])
        assert ov > 0.9, (s, ov)
        return m.e_tot + t.e[k]
    _fd_rule(f"{driver} state 1 on {xc} (omega = {td.e[0]:.6f} Ha, full-range call {tm['grad_jk_full_s']:.4f} s, "
             f"long-range call {tm['grad_jk_lr_s']:.4f} s)", g, u, energy, _eps(c))


def test_root_check_refuses_a_coupling_without_k_lr_and_a_shifted_root(world):
    """``grad_elec`` with ``rsh=None`` on the CAM-B3LYP root forms the global-hybrid coupling, hyb K alone: its
    omega misses the root by the long-range exchange of the state, and ``check_root`` refuses before any
    derivative is formed.  So does the full driver against a root shifted by 1e-6 Ha."""
    c = world("cam-b3lyp")
    mf = c["mf"]
    (make, _, _), _ = DRIVERS["sf_down_2"]
    td = make(mf)
    x = sf_amplitude(td, 0)
    tm = {}
    with pytest.raises(AssertionError, match="omega") as err:
        SFG.grad_elec(mf, x, False, mf._device, timings=tm, hyb=float(mf.hyb), xc=SFG.KSTerms(mf, (0, 1), tm),
                      rsh=None, root=float(td.e[0]))
    print(f"without K_LR: {err.value}")
    assert "zvector_s" not in tm                     # refused before the Z-vector
    gm = td.Gradients(state=1)
    td.e = np.asarray(td.e) + 1e-6
    with pytest.raises(AssertionError, match="omega"):
        gm.kernel()
