"""Host checks of the analytic gradients (no GPU): the one-electron derivatives against central
differences, the translational sum rules, the dense restatement ``tests/grad_ref.py`` (UHF,
spin-flip-down and -up CIS) against finite differences of the energies, the C entry's argument
checks and the refusals."""
import numpy as np
import pytest

import grad_ref as R
from xtddft_amd import _capi, build, qc
from xtddft_amd.qc import grad as G

EPS = np.finfo(np.float64).eps
H_FD = 2e-3       # Bohr


# --------------------------------------------------------------------------- one-electron derivatives
SPD = {"H": [[0, [4.0, 0.11], [1.1, 0.52], [0.35, 0.48]], [1, [0.8, 1.0]], [2, [0.7, 1.0]]]}
SPD_ATOMS = [("H", (0.0, 0.0, 0.0)), ("H", (0.0, 1.7, 1.1)), ("H", (1.3, -0.9, 0.6))]


@pytest.fixture(scope="module")
def spd_mol():
    return qc.M(SPD_ATOMS, basis=SPD, spin=1, unit="Bohr")


def _moved(mol, ia, x, step):
    u = np.zeros((mol.natm, 3))
    u[ia, x] = 1.0
    return R.displaced(mol, u, step)


def test_one_electron_derivatives_against_central_differences(spd_mol):
    """d/dR_A of int1e_ovlp / int1e_kin / int1e_nuc for every atom and direction: two Richardson
    estimates from the steps (2h, h) and (h, h/2); bound 10 x their difference + 2 eps max|integral| / h."""
    mol = spd_mol
    on = mol.ao_atom()
    s1, ik, hd = G.get_ovlp(mol), G.ipkin(mol), G.hcore_generator(mol)
    worst = {}
    for ia in range(mol.natm):
        rows = on == ia
        for x in range(3):
            ana = {}
            for name, d in (("int1e_ovlp", s1[x]), ("int1e_kin", -ik[x])):
                m = np.zeros_like(d)
                m[rows] = d[rows]
                ana[name] = m + m.T
            ana["int1e_nuc"] = hd(ia)[x] - ana["int1e_kin"]
            for name in ana:
                fine, coarse = R.richardson(lambda s: _moved(mol, ia, x, s).intor(name), H_FD)
                lhs = np.abs(ana[name] - fine).max()
                rhs = 10 * np.abs(fine - coarse).max() + 2 * EPS * np.abs(mol.intor(name)).max() / H_FD
                key = (name, lhs / rhs)
                if name not in worst or worst[name][1] < key[1]:
                    worst[name] = (f"atom {ia} dir {x}: {lhs:.2e} <= {rhs:.2e}", lhs / rhs)
                assert lhs <= rhs, (name, ia, x, lhs, rhs)
    for name, (txt, _) in worst.items():
        print(f"{name}: tightest case {txt}")


def test_translational_sum_rules(spd_mol):
    mol = spd_mol
    s1, ik, hd = G.get_ovlp(mol), G.ipkin(mol), G.hcore_generator(mol)
    vat = G.iprinv_atoms(mol)
    scale = np.abs(vat).max()
    # moving every centre together changes nothing: sum_A d/dR_A <mu|h|nu> = 0, and the operator
    # derivatives alone sum to minus the basis-function (electron-coordinate) derivatives
    tot = sum(hd(ia) for ia in range(mol.natm))
    assert np.abs(tot).max() < 1e-12 * scale
    ipnuc = vat.sum(axis=0)
    op = sum(vat[ia] + vat[ia].transpose(0, 2, 1) for ia in range(mol.natm))
    basis = -(ipnuc + ipnuc.transpose(0, 2, 1))
    assert np.abs(op + basis).max() < 1e-12 * scale
    assert np.abs(s1 + s1.transpose(0, 2, 1)).max() < 1e-13
    assert np.abs(ik + ik.transpose(0, 2, 1)).max() < 1e-12 * np.abs(ik).max()
    assert np.abs(G.grad_nuc(mol).sum(axis=0)).max() < 1e-13
    assert G.grad_nuc(mol, atmlst=[2, 0]).shape == (2, 3)


# --------------------------------------------------------------------------- restated gradients
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)


@pytest.fixture(scope="module")
def ch2():
    mol = qc.M(CH2, basis="6-31g", spin=2)
    mf = R.run_uhf(mol)
    return mol, mf, R.deriv_eri(mol)


@pytest.fixture(scope="module")
def ch2_fd(ch2):
    """The SCF and both spin-flip spectra at the displaced geometries of two fixed random
    directions (steps +-2h, +-h, +-h/2), computed once."""
    mol = ch2[0]
    out = {}
    for seed in (1, 2):
        u = R.random_direction(mol.natm, seed)
        for s in (2 * H_FD, H_FD, H_FD / 2):
            for sg in (1, -1):
                m = R.run_uhf(R.displaced(mol, u, sg * s))
                out[(seed, sg * s)] = (m.e_tot, m.last_energy_change, R.sf_states(m, -1), R.sf_states(m, 1))
    return out


def fd_check(g, u, energy, eps_e, what):
    """|g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2)."""
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"{what}: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= {rhs:.2e} "
          f"(Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs, (what, lhs, rhs)


@pytest.mark.parametrize("seed", [1, 2])
def test_restated_uhf_gradient_against_finite_differences(ch2, ch2_fd, seed):
    mol, mf, ip = ch2
    u = R.random_direction(mol.natm, seed)
    eps_e = max([mf.last_energy_change] + [v[1] for k, v in ch2_fd.items() if k[0] == seed])
    fd_check(R.uhf_grad(mf, ip), u, lambda s: ch2_fd[(seed, s)][0], eps_e, f"UHF dir {seed}")


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("isf", [-1, 1])
def test_restated_spin_flip_gradient_against_finite_differences(ch2, ch2_fd, isf, seed):
    """State 1 of spin-flip-down / -up CIS; the followed root keeps an overlap above 0.9 with the
    undisplaced state at every displaced geometry."""
    mol, mf, ip = ch2
    u = R.random_direction(mol.natm, seed)
    e0, xs, xao = R.sf_states(mf, isf)

    def energy(s):
        e_scf, _, down, up = ch2_fd[(seed, s)]
        e, _, xao_s = down if isf == -1 else up
        k, ov = R.follow(mf.s1e, xao[0], xao_s)
        assert ov > 0.9, (s, ov)
        return e_scf + e[k]
    eps_e = max([mf.last_energy_change] + [v[1] for k, v in ch2_fd.items() if k[0] == seed])
    fd_check(R.sf_grad(mf, xs[0], isf, ip), u, energy, eps_e, f"SF {'down' if isf == -1 else 'up'} state 1 dir {seed}")


# --------------------------------------------------------------------------- the C entry
def test_exports_and_build_lists():
    import os
    assert "xt_grad_jk" in _capi.EXPORTS
    assert "xt_grad.hip" in build.SOURCES and "xt_hint_dev.h" in build.HEADERS
    assert _capi.ABI_VERSION == 8
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        assert "int xt_grad_jk(" in f.read()


def test_xt_grad_jk_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with its own message before the first HIP call."""
    L = hiplib
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data

    def call(nbra=1, binfo=i, bprim=d, eb=d, bao=i, nket=1, kinfo=i, kprim=d, ek=d, kao=i, lbra=3, lket=2, nterm=2,
             wj=d, wk=d, p=d, q=d, nao=1, strip=1, natm=1, work=d, nwork=6, out=d):
        return L.xt_grad_jk(nbra, binfo, bprim, eb, bao, nket, kinfo, kprim, ek, kao, lbra, lket, nterm, wj, wk, p, q,
                            nao, strip, natm, work, nwork, out, None)

    def rejected(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.xt_last_error(), L.xt_last_error()
    for name in ("nbra", "nket", "nao", "natm", "nwork"):
        rejected(call(**{name: -1}), "negative size")
    rejected(call(strip=0), "strip")
    rejected(call(lbra=-1), "order")
    rejected(call(lket=-1), "order")
    rejected(call(lbra=9, lket=0), "order")
    rejected(call(lbra=8, lket=7), "order")
    rejected(call(lbra=7, lket=8), "order")
    rejected(call(nterm=0), "nterm")
    rejected(call(nterm=9), "nterm")
    rejected(call(wj=None), "null")
    rejected(call(wk=None), "null")
    for name in ("binfo", "bprim", "eb", "bao", "kinfo", "kprim", "ek", "kao", "p", "q", "work", "out"):
        rejected(call(**{name: None}), "null")
    rejected(call(nwork=5), "workspace")
    rejected(call(nket=5, strip=2, nwork=11), "workspace")        # 3 strips + 1: 12 doubles
    rejected(call(nket=5, strip=2**31 - 1, nwork=5), "workspace")  # no int overflow in the strip count
    assert call(nbra=0, binfo=None, out=None) == 0 and call(nket=0, kinfo=None) == 0      # nothing to add


# --------------------------------------------------------------------------- refusals
def test_refusals():
    from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up
    mol = qc.M(CH2, basis="6-31g", spin=2)
    with pytest.raises(NotImplementedError):
        qc.ROHF(mol).nuc_grad_method()
    with pytest.raises(NotImplementedError):
        qc.UKS(mol, xc="b3lyp").nuc_grad_method()
    with pytest.raises(NotImplementedError):
        qc.UHF(mol).density_fit().nuc_grad_method()
    ro = qc.ROHF(mol)
    ro.kernel()
    with pytest.raises(NotImplementedError):
        SF_TDA_down(ro.to_meanfield(), davidson=False).nuc_grad_method()
    uks = qc.UKS(mol, xc="b3lyp")
    uks.kernel()
    with pytest.raises(NotImplementedError):
        SF_TDA_down(uks.to_meanfield(), davidson=False).nuc_grad_method()
    df = qc.UHF(mol).density_fit()
    df.kernel()
    with pytest.raises(NotImplementedError):
        SF_TDA_up(df.to_meanfield(), davidson=False).nuc_grad_method()
    hf = qc.UHF(mol)
    hf.kernel()
    with pytest.raises(NotImplementedError):
        SF_TDA_down(hf.to_meanfield(), method=1, davidson=False).nuc_grad_method()
    g = SF_TDA_down(hf.to_meanfield(), davidson=False).nuc_grad_method()
    assert (g.state, g.cphf_conv_tol, g.atmlst) == (1, 1e-10, None) and g.cphf_max_cycle >= 20
    loose = qc.UHF(mol)
    loose.eri_mode, loose.chol_tol = "cholesky", 1e-6      # approximate J / K against exact derivative integrals
    with pytest.raises(ValueError):
        loose.nuc_grad_method()
    with pytest.raises(RuntimeError):          # no quiet host fall-back: the hot path is the device kernel
        hf.nuc_grad_method().kernel()
