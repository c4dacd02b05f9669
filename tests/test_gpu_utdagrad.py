"""GPU: the U-TDA gradient ``XTDA(mol, mf).nuc_grad_method()`` (xtddft_amd/grad_utda.py) on CH2
triplet against the NumPy restatement ``tests/utdagrad_ref.py`` and against finite differences of the
device's own E_SCF + omega on a grid frozen in space, the Davidson route against the dense one, and
the neighbours that share cached state with it (``fxc_ground``, the gradient tables).

The Kohn-Sham cases run on every fourth point of the level-3 grid (``ksgrad_ref.coarse_grids``): the
gradient is the exact derivative of the energy on whatever fixed set of points and weights the mean
field carries, and the restatement's explicit third-derivative tensor stays small.  Translational sums
do not vanish on a frozen grid and are asserted for Hartree-Fock only."""
import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
import sfksgrad_ref as SK
import utdagrad_ref as UR
from xtddft_amd import qc
from xtddft_amd.grad_utda import UTDAGradients, utda_amplitudes
from xtddft_amd.sf_tda import SF_TDA_down
from xtddft_amd.xtda import XTDA

pytestmark = pytest.mark.gpu

H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)
STRIDE = 4


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _device_scf(mol, xc, grids=None):
    mf = qc.UHF(mol) if xc == "hf" else qc.UKS(mol, xc=xc)
    if xc != "hf":
        mf.grids = grids             # build() keeps a grid that is already set
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


def _states(mf, davidson=False, nstates=4):
    td = XTDA(mf.mol, mf.to_meanfield(), nstates=nstates, use_Davidson=davidson)
    if davidson:
        td.conv_tol, td.lindep = 1e-8, 1e-20       # residual norm below 1e-8; no correction vector dropped above it
    td.kernel()
    return td


def _xao(mf, td, root):
    x = utda_amplitudes(td, root)
    return UR.xao(mf, x)


@pytest.fixture(scope="module")
def world(torch):
    """Per basis: the molecule, its dense derivative ERIs and its frozen grid; per (basis, functional): the
    device mean field, the restatement's XC arrays and third derivative, its Z-vector matrix, the
    dense U-TDA solution of the device."""
    mols, cases = {}, {}

    def mol_of(basis):
        if basis not in mols:
            mol = qc.M(CH2, basis=basis, spin=2)
            mols[basis] = (mol, R.deriv_eri(mol), K.coarse_grids(mol, STRIDE), {})
        return mols[basis]

    def case(basis, xc):
        if (basis, xc) not in cases:
            mol, ip, grids, shared = mol_of(basis)
            mf = _device_scf(mol, xc, grids)
            if xc == "hf":
                xa, kxc = SK.zero_xc_arrays(mol.nao), UR.zero_kxc()
            else:
                if "ao10" not in shared:
                    shared["ao10"] = K.ao_deriv2(mol, grids.coords)
                xa = SK.xc_arrays(mf, shared["ao10"])
                kxc = UR.kxc_arrays(mf, xa)
            cases[(basis, xc)] = dict(mol=mol, ip=ip, mf=mf, xa=xa, kxc=kxc, mcache={}, td=_states(mf))
        return cases[(basis, xc)]
    return case


CASES = [("6-31g", "hf"), ("6-31g", "svwn"), ("6-31g", "pbe"), ("6-31g", "b3lyp"), ("cc-pvdz", "b3lyp")]


@pytest.mark.parametrize("state", [1, 2])
@pytest.mark.parametrize("basis,xc", CASES)
def test_gradient_against_restatement(world, basis, xc, state):
    """Dense route, states 1 and 2: |g - restatement| <= 1e-8, Z-vector residual <= 1e-10, the device's
    excitation energies equal to the restatement's to 1e-8; UHF: |sum_A g_A| <= 1e-9.  cc-pVDZ puts the d
    bucket and the uncached Gamma path under the full pair lists (three Coulomb, eight exchange)."""
    c = world(basis, xc)
    mol, mf, td = c["mol"], c["mf"], c["td"]
    e_ref, _ = UR.utda_states(mf, c["xa"])
    assert np.abs(np.asarray(td.e)[:4] - e_ref[:4]).max() <= 1e-8
    gm = td.nuc_grad_method()
    assert isinstance(gm, UTDAGradients) and gm.is_ks == (xc != "hf")
    g = gm.kernel(state=state)
    tm = dict(gm.timings)
    x = utda_amplitudes(td, state - 1)
    ref, S, parts = UR.utda_grad(mf, x, c["ip"], c["xa"], c["kxc"], mcache=c["mcache"])
    assert abs(parts["omega"] - td.e[state - 1]) <= 1e-8
    print(f"U-TDA state {state} on {xc} / {basis}: omega = {td.e[state - 1]:.6f}, max|g| = {np.abs(ref).max():.4e}, "
          f"max|g_xc| = {np.abs(parts['xc']).max():.3e}, max|third-derivative part| = {np.abs(parts['xc_kxc']).max():.3e}, "
          f"max|device - restatement| = {np.abs(g - ref).max():.2e}, Z-vector {tm['zvector_cycles']} cycles, residual "
          f"{tm['zvector_residual']:.1e}, grad_jk_s = {tm['grad_jk_s']:.3f} over {len(tm['buckets'])} launches; "
          f"sum_A g = {g.sum(axis=0)}")
    assert g.shape == (3, 3) and len(tm["buckets"]) > 0
    if basis == "cc-pvdz":
        assert max(b["bra_order"] for b in tm["buckets"]) >= 5          # the d bucket ran
    assert tm["zvector_residual"] <= 1e-10
    assert np.abs(g - ref).max() <= 1e-8
    if xc == "hf":
        assert np.abs(g.sum(axis=0)).max() <= 1e-9
    else:
        assert np.abs(gm.de_xc - parts["xc"]).max() <= 1e-8
    if state == 1:
        assert td.nuc_grad_method().kernel(state=1, atmlst=[2]).tobytes() == g[2:3].tobytes()


@pytest.mark.parametrize("xc", ["hf", "b3lyp"])
def test_gradient_against_device_frozen_grid_finite_differences(world, xc):
    """State 1, e_tot + omega from the device drivers with the undisplaced grid, one seeded direction, the
    root followed by overlap: |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr."""
    c = world("6-31g", xc)
    mol, mf, td = c["mol"], c["mf"], c["td"]
    g = td.nuc_grad_method().kernel(state=1)
    u = R.random_direction(mol.natm, 3)
    grids = mf.grids if xc != "hf" else None
    fd = {sg * s: _device_scf(R.displaced(mol, u, sg * s), xc, grids) for s in (2 * H_FD, H_FD, H_FD / 2) for sg in (1, -1)}
    x0 = _xao(mf, td, 0)

    def energy(s):
        m = fd[s]
        assert xc == "hf" or m.grids is mf.grids
        t = _states(m, nstates=6)
        k, ov = UR.follow(mf.s1e, x0, [_xao(m, t, r) for r in range(6)])
        assert ov > 0.9, (s, ov)
        return m.e_tot + t.e[k]
    eps_e = max([abs(mf.last_energy_change)] + [abs(m.last_energy_change) for m in fd.values()])
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"U-TDA state 1 on {xc}: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} "
          f"<= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs


def test_davidson_route_gives_the_dense_gradient(world):
    """State 1 from Davidson amplitudes: the gradient differs from the dense route's by at most ten times
    the root's residual norm against the dense A; a root flagged unconverged is refused."""
    c = world("6-31g", "b3lyp")
    mf, dense = c["mf"], c["td"]
    td = _states(mf, davidson=True, nstates=2)
    assert bool(np.asarray(td.converged)[0])
    A = dense.A
    v = np.asarray(td.v)[:, 0]
    v = v / np.linalg.norm(v)
    resid = np.linalg.norm(A @ v - (v @ A @ v) * v)
    g = td.nuc_grad_method().kernel(state=1)
    diff = np.abs(g - dense.nuc_grad_method().kernel(state=1)).max()
    print(f"Davidson route U-TDA on UKS b3lyp: residual norm {resid:.2e}, max gradient difference {diff:.2e}")
    assert diff <= 10 * resid
    td.converged = np.array([False, False])
    with pytest.raises(RuntimeError):
        td.nuc_grad_method().kernel(state=1)


def test_neighbours_keep_their_bits(world):
    """The ground-state gradients and a spin-flip gradient of the same mean fields, before and after a
    ``UTDAGradients.kernel()`` in the same process: equal bits (``fxc_ground`` and the gradient tables are
    shared and must not be changed by it)."""
    for xc in ("hf", "b3lyp"):
        c = world("6-31g", xc)
        mf, td = c["mf"], c["td"]
        sf = SF_TDA_down(mf.to_meanfield(), method=0 if xc == "hf" else 2, davidson=False)
        sf.kernel(nstates=2)

        def both():
            return mf.nuc_grad_method().kernel().tobytes(), sf.nuc_grad_method().kernel(state=1).tobytes()
        before = both()
        g = td.nuc_grad_method().kernel(state=2)
        assert np.isfinite(g).all()
        assert both() == before, xc


def test_fxc_response_rho1_leaves_v_and_wv_unchanged(world, torch):
    c = world("6-31g", "b3lyp")
    mf = c["mf"]
    eng = mf.device_engine
    eng.fxc_ground(mf.make_rdm1())
    rng = np.random.default_rng(2)
    dm = rng.standard_normal((2, mf.mol.nao, mf.mol.nao)) * 0.1
    dm = dm + dm.transpose(0, 2, 1)
    two = eng.fxc_response(dm, want=("v", "wv"))
    three = eng.fxc_response(dm, want=("v", "wv", "rho1"))
    assert set(three) == {"v", "wv", "rho1"}
    assert three["v"].tobytes() == two["v"].tobytes() and torch.equal(three["wv"], two["wv"])
    r1 = three["rho1"].cpu().numpy()
    ref = np.einsum('gm,smn,gn->sg', c["xa"].ao10[0], dm, c["xa"].ao10[0])
    assert r1.shape == (2, 4, mf.grids.size) and np.abs(r1[:, 0] - ref).max() <= 1e-12 * np.abs(ref).max()
    with pytest.raises(ValueError):
        eng.fxc_response(dm, want=("rho",))
