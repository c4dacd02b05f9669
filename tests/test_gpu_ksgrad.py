"""GPU: the XC force kernel ``xt_grad_xc`` (xtddft_amd/csrc/xt_grad_xc.hip) on hand-built shell
tables with random h, e, c against the NumPy restatement ``tests/ksgrad_ref.py``, and the UKS
ground-state gradient on the device (``qc.grad.KSGradients``) against the restatement and against
finite differences of device energies on a grid frozen in space.

Raw calls are compared elementwise inside 1e-12 S, S being the sum of the absolute values of every
summed term (``ksgrad_ref.xc_bracket``): the bound ``xt_grad_jk`` is held to against its
restatement, on a scale that cancellation cannot shrink.  Translational invariance of the XC part
does not hold without weight derivatives and is not asserted; sum_A g[A] is printed."""
import numpy as np
import pytest

import grad_ref as R
import ksgrad_ref as K
from xtddft_amd import _capi, qc
from xtddft_amd.qc import grad as G
from xtddft_amd.qc.dints import _sph_table, ao_shell_tables

pytestmark = pytest.mark.gpu

H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)
GRIDS = (1, 63, 64, 65, 300)     # 300 leaves a remainder in the 64-point (GGA) and the 256-point (LDA) tile
EXPS = {1: ([0.8], [1.0]), 3: ([4.0, 1.1, 0.35], [0.11, 0.52, 0.48])}


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _shell(atom, l, nprim, centre=None):
    e = np.asarray(EXPS[nprim][0], dtype=np.float64)
    c = np.asarray(EXPS[nprim][1], dtype=np.float64) * qc.gto.gto_norm(l, e)
    return qc.gto.Shell(atom, l, np.array(R.CENTRES[atom] if centre is None else centre, dtype=np.float64), e, c)


def single(l, nprim):
    return R.ShellMol([_shell(1, l, nprim)], 3)


def mixed(atoms=(0, 1, 2, 0, 1), natm=3):
    """s .. g on three centres, contracted s and d; ``atoms``: the row each shell folds into."""
    ls, nps, ctr = (0, 1, 2, 3, 4), (3, 1, 3, 1, 1), (0, 1, 2, 0, 1)
    return R.ShellMol([_shell(a, l, n, R.CENTRES[c]) for a, l, n, c in zip(atoms, ls, nps, ctr)], natm)


def points(ng, seed):
    rng = np.random.default_rng(seed)
    return R.CENTRES[rng.integers(0, 3, ng)] + rng.uniform(-2.0, 2.0, (ng, 3))


def operands(mol, ng, nspin, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nspin, 4, ng)), rng.standard_normal((nspin, mol.nao, ng)),
            rng.standard_normal((nspin, mol.nao, ng)))


def raw_call(torch, hiplib, mol, coords, h, e, c, gga, out0=None, lmax=None):
    """One xt_grad_xc call; h (nspin, 4, G), e, c (nspin, nao, G) as the kernel reads them."""
    dv = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.ascontiguousarray(x), device=dv)
    info, dat = ao_shell_tables(mol)
    ng, nspin, nshell = coords.shape[0], e.shape[0], len(mol.shells)
    dev = [t(coords), t(info), t(dat), t(_sph_table()), t(mol._norm),
           t(np.array([s.atom for s in mol.shells], dtype=np.int32)), t(h), t(e), t(c)]
    out = t(np.zeros((mol.natm, 3)) if out0 is None else out0)
    nwork = G.xc_work_size(ng, nshell)
    work = torch.full((nwork,), float("nan"), dtype=torch.float64, device=dv)
    rc = hiplib.xt_grad_xc(ng, dev[0].data_ptr(), nshell, *[x.data_ptr() for x in dev[1:6]],
                           max(s.l for s in mol.shells) if lmax is None else lmax, mol.natm, mol.nao, nspin,
                           _capi.XC["GGA" if gga else "LDA"], *[x.data_ptr() for x in dev[6:]], ng,
                           work.data_ptr(), nwork, out.data_ptr(), None)
    _capi.check(rc, "xt_grad_xc")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(torch, hiplib, mol, coords, seed, what, nspins=(1, 2), modes=(False, True)):
    """Every (nspin, mode) at these points against the restatement; returns the largest error / S."""
    ao10 = K.ao_deriv2(mol, coords)
    worst = 0.0
    for nspin in nspins:
        h, e, c = operands(mol, coords.shape[0], nspin, seed)
        for gga in modes:
            ref, S = K.xc_bracket(ao10, mol.ao_atom(), mol.natm, h, e, c, gga)
            got = raw_call(torch, hiplib, mol, coords, h, e, c, gga)
            err = np.abs(got - ref).max()
            worst = max(worst, err / S)
            assert np.isfinite(got).all() and np.abs(ref).max() > 0
            assert err <= 1e-12 * S, (what, coords.shape[0], nspin, gga, err, S)
    return worst


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("nprim", [1, 3])
@pytest.mark.parametrize("l", [0, 1, 2, 3, 4])
def test_kernel_per_l_against_restatement(torch, hiplib, l, nprim):
    mol = single(l, nprim)
    worst = max(check(torch, hiplib, mol, points(ng, 10 * l + ng), 7 + l, f"l = {l}") for ng in GRIDS)
    print(f"l = {l}, nprim = {nprim}: largest |kernel - restatement| / S = {worst:.2e} over grids {GRIDS}, "
          f"nspin 1 / 2, LDA / GGA")


def test_kernel_mixed_set_on_three_centres(torch, hiplib):
    mol = mixed()
    assert mol.nao == 25 and sorted(s.l for s in mol.shells) == [0, 1, 2, 3, 4]
    worst = max(check(torch, hiplib, mol, points(ng, ng), 3, "mixed") for ng in GRIDS)
    print(f"s..g on three centres: largest |kernel - restatement| / S = {worst:.2e} over grids {GRIDS}")


def test_kernel_degenerate_points(torch, hiplib):
    """Points on every nucleus and on the coordinate planes and axes through one (the ix = 0 / 1
    branches of the polynomial derivatives), and points 40 Bohr away, where the radial part has
    underflowed for every exponent but the most diffuse one (0.35): finite, and inside the bound.  A
    shell whose only exponent (0.8) has underflowed at all its points gives exactly zero."""
    mol = mixed()
    c = R.CENTRES
    near = np.concatenate([c, c[1] + np.array([[0.7, 0, 0], [0, -0.4, 0], [0, 0, 1.1], [0.3, 0.5, 0], [0, 0.2, -0.6],
                                               [-0.9, 0, 0.8]])])
    far = c[0] + 40.0 * np.array([[1.0, 0, 0], [0, -1.0, 0], [0.6, 0, 0.8]])
    worst = check(torch, hiplib, mol, np.concatenate([near, far]), 11, "degenerate")
    print(f"degenerate points: largest |kernel - restatement| / S = {worst:.2e}")
    one = single(2, 1)
    h, e, cc = operands(one, 3, 2, 5)
    for gga in (False, True):      # nothing but underflowed points: zero, not NaN
        assert np.array_equal(raw_call(torch, hiplib, one, far, h, e, cc, gga), np.zeros((3, 3)))


def test_lda_mode_reads_neither_c_nor_h(torch, hiplib):
    """LDA mode with c and every plane of h filled with NaN gives the finite LDA answer bit for
    bit; GGA mode never reads plane 0 of h (it is part of e)."""
    mol = mixed()
    coords = points(130, 2)
    h, e, c = operands(mol, 130, 2, 4)
    nan = np.full_like
    lda = raw_call(torch, hiplib, mol, coords, h, e, c, False)
    got = raw_call(torch, hiplib, mol, coords, nan(h, np.nan), e, nan(c, np.nan), False)
    assert np.isfinite(got).all() and got.tobytes() == lda.tobytes()
    h0 = h.copy()
    h0[:, 0] = np.nan
    gga = raw_call(torch, hiplib, mol, coords, h, e, c, True)
    assert raw_call(torch, hiplib, mol, coords, h0, e, c, True).tobytes() == gga.tobytes()
    assert np.abs(gga - lda).max() > 1e-3


def test_rows_determinism_accumulation_and_declared_lmax(torch, hiplib):
    mol3 = mixed()
    mol2 = mixed(atoms=(0, 1, 0, 0, 1), natm=2)       # the centre of atom 2 now folds into row 0
    coords = points(300, 9)
    ao10 = K.ao_deriv2(mol3, coords)
    h, e, c = operands(mol3, 300, 2, 6)
    ref3, S = K.xc_bracket(ao10, mol3.ao_atom(), 3, h, e, c, True)
    ref2, _ = K.xc_bracket(ao10, mol2.ao_atom(), 2, h, e, c, True)
    a3 = raw_call(torch, hiplib, mol3, coords, h, e, c, True)
    a2 = raw_call(torch, hiplib, mol2, coords, h, e, c, True)
    assert np.abs(a2 - ref2).max() <= 1e-12 * S and np.abs(a3 - ref3).max() <= 1e-12 * S
    assert np.abs(a2[0] - (a3[0] + a3[2])).max() <= 1e-12 * S and a2[1].tobytes() == a3[1].tobytes()
    # two identical calls: identical bytes
    assert raw_call(torch, hiplib, mol3, coords, h, e, c, True).tobytes() == a3.tobytes()
    assert raw_call(torch, hiplib, mol3, coords, h, e, c, False).tobytes() == \
        raw_call(torch, hiplib, mol3, coords, h, e, c, False).tobytes()
    # out is accumulated into: out0 + (the sum from a zeroed out), one rounding
    out0 = np.random.default_rng(1).standard_normal((3, 3))
    assert raw_call(torch, hiplib, mol3, coords, h, e, c, True, out0=out0).tobytes() == (out0 + a3).tobytes()
    # a shell above the declared lmax adds nothing: lmax = 2 leaves the s, p, d shells
    low = R.ShellMol(mol3.shells[:3], 3)
    b = raw_call(torch, hiplib, mol3, coords, h, e, c, True, lmax=2)
    refl, Sl = K.xc_bracket(ao10[:, :, :low.nao], low.ao_atom(), 3, h, e[:, :low.nao], c[:, :low.nao], True)
    assert np.abs(b - refl).max() <= 1e-12 * Sl


# --------------------------------------------------------------------------- CH2 / cc-pVDZ on the device
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


@pytest.fixture(scope="module")
def ch2(hiplib):
    mol = qc.M(CH2, basis="cc-pvdz", spin=2)
    assert mol.nao == 24
    return mol, R.deriv_eri(mol), {}


def _mf(ch2, xc):
    mol, _, cache = ch2
    if xc not in cache:
        cache[xc] = _device_uks(mol, xc, cache[next(iter(cache))].grids if cache else None)
    return cache[xc]


@pytest.mark.parametrize("xc", ["svwn", "pbe", "b3lyp"])
def test_uks_gradient_on_device_against_restatement(ch2, xc):
    """LDA, a pure GGA (the J-only two-electron path) and a hybrid GGA."""
    mol, ip, _ = ch2
    mf = _mf(ch2, xc)
    gm = mf.nuc_grad_method()
    assert isinstance(gm, G.KSGradients)
    g = gm.kernel()
    ref, S, parts = K.uks_grad(mf, ip)
    print(f"UKS {xc} CH2 / cc-pVDZ ({mf.grids.size} points): max|g| = {np.abs(ref).max():.4e}, max|g_xc| = "
          f"{np.abs(parts['xc']).max():.4e}, S = {S:.3e}, max|device - restatement| = {np.abs(g - ref).max():.2e}, "
          f"max|g_xc device - restatement| = {np.abs(gm.de_xc - parts['xc']).max():.2e}, sum_A g = {g.sum(axis=0)}")
    assert g.shape == (3, 3)
    assert len(G.ks_ground_terms(np.eye(2), np.eye(2), mf.hyb)) == (3 if xc == "b3lyp" else 1)
    assert np.abs(g - ref).max() <= 1e-9
    assert np.abs(mf.nuc_grad_method().kernel(atmlst=[2]) - g[2]).max() == 0.0
    assert np.abs(g[:, 0]).max() <= 1e-10                            # out of the molecular plane


def test_chunked_grid_loop_equals_the_unchunked(ch2):
    """A chunk that splits the grid unevenly changes the summation order only."""
    mf = _mf(ch2, "b3lyp")
    d = [mf.mo_coeff[s][:, mf.mo_occ[s] > 0] @ mf.mo_coeff[s][:, mf.mo_occ[s] > 0].T for s in range(2)]
    ng = mf.grids.size
    st = {}
    whole = G.grad_xc_device(mf, d[0], d[1], chunk=ng, stats=st)
    assert st["chunks"] == 1 and G.default_xc_chunk(mf.mol.nao, ng) == ng      # the default here: one chunk
    assert G.default_xc_chunk(2000, 10**7) == 4096 and G.default_xc_chunk(10**6, 10**7) == 256
    for chunk in (10007, 3000):
        assert ng % chunk and chunk % 64
        st = {}
        part = G.grad_xc_device(mf, d[0], d[1], chunk=chunk, stats=st)
        err = np.abs(part - whole).max() / np.abs(whole).max()
        print(f"chunk {chunk} ({st['chunks']} chunks of {ng} points): relative difference {err:.2e}")
        assert st["chunks"] == -(-ng // chunk) and err <= 1e-13


def test_uks_gradient_against_device_frozen_grid_finite_differences(ch2):
    """B3LYP, device energies with the undisplaced grid, one random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr, eps_E the
    largest last_energy_change of the runs involved."""
    mol = ch2[0]
    mf = _mf(ch2, "b3lyp")
    g = mf.nuc_grad_method().kernel()
    u = R.random_direction(mol.natm, 3)
    runs = {}
    for s in (2 * H_FD, H_FD, H_FD / 2):
        for sg in (1, -1):
            m = _device_uks(R.displaced(mol, u, sg * s), "b3lyp", mf.grids)
            assert m.grids is mf.grids
            runs[sg * s] = (m.e_tot, m.last_energy_change)
    eps_e = max([mf.last_energy_change] + [v[1] for v in runs.values()])
    fine, coarse = R.richardson(lambda s: runs[s][0], H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"UKS b3lyp: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} <= {rhs:.2e} "
          f"(Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs
