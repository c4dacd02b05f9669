"""GPU: the derivative-ERI contraction kernel ``xt_grad_jk`` (xtddft_amd/csrc/xt_grad.hip), the UHF
gradient and the spin-flip CIS gradients on the device against the dense restatement
``tests/grad_ref.py`` and against finite differences of the device energies."""
import numpy as np
import pytest

import grad_ref as R
from xtddft_amd import qc
from xtddft_amd.grad import sf_amplitude
from xtddft_amd.qc import grad as G
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up

pytestmark = pytest.mark.gpu

H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)
SF = {-1: SF_TDA_down, 1: SF_TDA_up}


# --------------------------------------------------------------------------- the kernel
def _terms(n, seed, nterm=2):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(0.5, 1.5)), float(rng.uniform(-1.5, -0.5)), rng.standard_normal((n, n)),
             rng.standard_normal((n, n))) for _ in range(nterm)]


@pytest.fixture(scope="module")
def kernel_cases(hiplib):
    """Per dispatch bucket: the shell set, the dense derivative ERIs and random non-symmetric
    (P_t, Q_t), nterm = 2, whose contraction is not a cancellation artefact (checked on the CPU:
    max|g| >= 1e-2 sum|terms|)."""
    out = {}
    for kind in ("sp", "spd", "sf"):
        mol = R.shell_set(kind)
        ip = R.deriv_eri(mol)
        for seed in range(20):
            terms = _terms(mol.nao, seed)
            ref, mag = R.gamma_contract(mol, ip, terms, parts=True)
            if np.abs(ref).max() >= 1e-2 * mag:
                break
        else:
            raise AssertionError("no seed without cancellation")
        out[kind] = (mol, ip, terms, ref)
    return out


@pytest.mark.parametrize("kind,bra_order,tot_order", [("sp", 3, 5), ("spd", 5, 9), ("sf", 7, 13)])
def test_kernel_against_dense_restatement(kernel_cases, kind, bra_order, tot_order):
    mol, _, terms, ref = kernel_cases[kind]
    tab = G.grad_tables(mol)
    assert tab.bra_ranges[-1][2] == bra_order and tab.bra_ranges[-1][2] + tab.ket_ranges[-1][2] == tot_order
    assert any(i == j for i, j in tab.ket.pairs) and any(i != j for i, j in tab.ket.pairs)
    st = {}
    got = G.grad_jk_device(mol, terms, 0, stats=st)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{kind}: max|g| = {np.abs(ref).max():.3e}, relative error {err:.2e}, launches "
          f"{[(b['bra_order'], b['ket_order'], b['quartets']) for b in st['buckets']]}")
    assert err <= 1e-12


@pytest.mark.parametrize("kind", ["sp", "spd", "sf"])
def test_kernel_determinism_strips_and_linearity(kernel_cases, kind):
    mol, _, terms, ref = kernel_cases[kind]
    scale = np.abs(ref).max()
    a = G.grad_jk_device(mol, terms, 0)
    b = G.grad_jk_device(mol, terms, 0)
    assert a.tobytes() == b.tobytes()
    # the last strip length holds every ket of a launch in one strip ('sf': at most 3 kets per launch)
    for strip in ((2, 3) if kind == "sf" else (2, 3, 1000)):
        c = G.grad_jk_device(mol, terms, 0, strip=strip)
        assert np.abs(c - a).max() <= 1e-13 * scale, strip
    j_only = G.grad_jk_device(mol, [(wj, 0.0, P, Q) for wj, wk, P, Q in terms], 0)
    k_only = G.grad_jk_device(mol, [(0.0, wk, P, Q) for wj, wk, P, Q in terms], 0)
    assert np.abs(j_only).max() > 0 and np.abs(k_only).max() > 0
    assert np.abs(j_only + k_only - a).max() <= 1e-13 * scale


def test_kernel_term_count_limits(kernel_cases):
    mol, ip, terms, _ = kernel_cases["sp"]
    eight = _terms(mol.nao, 7, nterm=8)
    got = G.grad_jk_device(mol, eight, 0)
    ref = R.gamma_contract(mol, ip, eight)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    with pytest.raises(ValueError):
        G.grad_jk_device(mol, _terms(mol.nao, 7, nterm=9), 0)


# --------------------------------------------------------------------------- CH2 / cc-pVDZ on the device
def _device_uhf(mol):
    mf = qc.UHF(mol)
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


def _device_states(mf, isf):
    """Dense route on the device: explicit A (get_Amat) + eigh."""
    td = SF[isf](mf.to_meanfield(), method=0, davidson=False)
    td.kernel(nstates=2)
    return td


def _xao(mf, td, root):
    s = (0, 1) if td.isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    return cv @ sf_amplitude(td, root) @ co.T


@pytest.fixture(scope="module")
def ch2(hiplib):
    mol = qc.M(CH2, basis="cc-pvdz", spin=2)
    assert mol.nao == 24
    mf = _device_uhf(mol)
    return mol, mf, R.deriv_eri(mol), {isf: _device_states(mf, isf) for isf in (-1, 1)}


def test_uhf_gradient_on_device_against_restatement(ch2):
    mol, mf, ip, _ = ch2
    g = mf.nuc_grad_method().kernel()
    ref = R.uhf_grad(mf, ip)
    print(f"UHF CH2 / cc-pVDZ: max|g| = {np.abs(ref).max():.4e}, max|device - restatement| = {np.abs(g - ref).max():.2e}")
    assert g.shape == (3, 3)
    assert np.abs(g - ref).max() <= 1e-9
    assert np.abs(mf.nuc_grad_method().kernel(atmlst=[2]) - g[2]).max() == 0.0


@pytest.fixture(scope="module")
def ch2_sf_gradients(ch2):
    mol, mf, ip, tds = ch2
    out = {}
    for isf, td in tds.items():
        gm = td.nuc_grad_method()
        for state in (1, 2):
            out[(isf, state)] = (gm.kernel(state=state), dict(gm.timings))
    return out


@pytest.mark.parametrize("state", [1, 2])
@pytest.mark.parametrize("isf", [-1, 1])
def test_sf_gradient_against_restatement_and_invariances(ch2, ch2_sf_gradients, isf, state):
    mol, mf, ip, tds = ch2
    g, tm = ch2_sf_gradients[(isf, state)]
    ref = R.sf_grad(mf, sf_amplitude(tds[isf], state - 1), isf, ip)
    print(f"SF {isf:+d} state {state}: max|g| = {np.abs(ref).max():.4e}, max|device - restatement| = "
          f"{np.abs(g - ref).max():.2e}, Z-vector {tm['zvector_cycles']} cycles, residual {tm['zvector_residual']:.1e}")
    assert tm["zvector_residual"] <= 1e-10
    assert np.abs(g - ref).max() <= 1e-8
    Rc = mol.atom_coords()
    assert np.abs(g.sum(axis=0)).max() <= 1e-9                       # translation
    assert np.abs(np.cross(Rc, g).sum(axis=0)).max() <= 1e-9         # rotation
    assert np.abs(g[:, 0]).max() <= 1e-10                            # out of the molecular plane


@pytest.fixture(scope="module")
def ch2_fd(ch2):
    """Device SCF and both dense spin-flip spectra at the six displaced geometries of one random
    direction."""
    mol = ch2[0]
    u = R.random_direction(mol.natm, 3)
    out = {}
    for s in (2 * H_FD, H_FD, H_FD / 2):
        for sg in (1, -1):
            m = _device_uhf(R.displaced(mol, u, sg * s))
            out[sg * s] = (m, {isf: _device_states(m, isf) for isf in (-1, 1)})
    return u, out


@pytest.mark.parametrize("state", [1, 2])
@pytest.mark.parametrize("isf", [-1, 1])
def test_sf_gradient_against_device_finite_differences(ch2, ch2_sf_gradients, ch2_fd, isf, state):
    """|g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr, the
    followed root overlapping the undisplaced state by more than 0.9 at every geometry."""
    mol, mf, _, tds = ch2
    u, fd = ch2_fd
    g = ch2_sf_gradients[(isf, state)][0]
    x0 = _xao(mf, tds[isf], state - 1)

    def energy(s):
        m, t = fd[s]
        td = t[isf]
        xs = np.asarray([_xao(m, td, r) for r in range(min(6, np.asarray(td.v).shape[1]))])
        k, ov = R.follow(mf.s1e, x0, xs)
        assert ov > 0.9, (s, ov)
        return m.e_tot + td.e[k]
    eps_e = max([mf.last_energy_change] + [m.last_energy_change for m, _ in fd.values()])
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"SF {isf:+d} state {state}: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= "
          f"{rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs


@pytest.mark.parametrize("isf", [-1, 1])
def test_davidson_route_gives_the_dense_gradient(ch2, ch2_sf_gradients, isf):
    """State 1 from Davidson amplitudes converged to a residual of 1e-8 (``tol_residual``): the
    gradient differs from the dense route's by the first-order error of a non-converged amplitude,
    bounded by ten times the root's residual norm |A v - (v.A v) v| against the dense A."""
    mol, mf, _, tds = ch2
    td = SF[isf](mf.to_meanfield(), method=0, davidson=True, conv_tol=1e-14, tol_residual=1e-8, lindep=1e-20)
    td.kernel(nstates=2)
    assert bool(np.asarray(td.converged)[0])
    A = tds[isf].A
    v = np.asarray(td.v)[:, 0]
    v = v / np.linalg.norm(v)
    resid = np.linalg.norm(A @ v - (v @ A @ v) * v)
    g = td.nuc_grad_method().kernel(state=1)
    diff = np.abs(g - ch2_sf_gradients[(isf, 1)][0]).max()
    print(f"Davidson route SF {isf:+d}: residual norm {resid:.2e}, max gradient difference {diff:.2e}")
    assert resid <= 1e-8
    assert diff <= 10 * resid


def test_unconverged_davidson_root_is_refused(ch2):
    mol, mf, _, _ = ch2
    td = SF_TDA_down(mf.to_meanfield(), method=0, davidson=True)
    td.kernel(nstates=1)
    td.converged = np.array([False])
    with pytest.raises(RuntimeError):
        td.nuc_grad_method().kernel(state=1)


# --------------------------------------------------------------------------- the reference's own case
def test_n2_cation_spin_flip_down_gradient(hiplib):
    """usfcis.py:373-386: N2+ at 0.97 Angstrom, UHF conv_tol 1e-12, spin-flip-down state 1.  The
    reference runs 6-31G; the embedded 6-31G has no nitrogen entry, so this runs cc-pVDZ.  The
    reference stores no printed gradient: the check is symmetry and finite differences."""
    with pytest.raises(KeyError):
        qc.M("N 0 0 0; N 0 0 0.97", basis="6-31g", charge=1, spin=1)
    mol = qc.M("N 0 0 0; N 0 0 0.97", basis="cc-pvdz", charge=1, spin=1)
    mf = _device_uhf(mol)
    td = _device_states(mf, -1)
    g = td.nuc_grad_method().kernel(state=1)
    print(f"N2+ / cc-pVDZ SF-down state 1 gradient:\n{g}")
    assert np.abs(g[:, :2]).max() <= 1e-9 and abs(g[0, 2] + g[1, 2]) <= 1e-9 and abs(g[0, 2]) > 1e-4
    u = np.array([[0, 0, -1.0], [0, 0, 1.0]]) / np.sqrt(2)
    x0 = _xao(mf, td, 0)
    eps = [mf.last_energy_change]

    def energy(s):
        m = _device_uhf(R.displaced(mol, u, s))
        t = _device_states(m, -1)
        eps.append(m.last_energy_change)
        xs = np.asarray([_xao(m, t, r) for r in range(6)])
        k, ov = R.follow(mf.s1e, x0, xs)
        assert ov > 0.9, (s, ov)
        return m.e_tot + t.e[k]
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * max(eps) / (H_FD / 2)
    print(f"g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= {rhs:.2e}")
    assert lhs <= rhs
    # g_z(N1) = -g_z(N2) = -(g.u) / sqrt 2: both components equal the finite-difference value
    assert abs(-g[0, 2] * np.sqrt(2) - fine) <= rhs and abs(g[1, 2] * np.sqrt(2) - fine) <= rhs
