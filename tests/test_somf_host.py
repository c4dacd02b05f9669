"""Host: the derivative Hermite tables (qc/ints.py deriv_tables / DerivPair), the one-electron
integrals int1e_pnucp / int1e_wso, the host restatement of the spin-orbit mean field
(xtddft_amd/somf.py) and the sf-X2C mean field -- no GPU.

The l-shift bound.  A derivative block is compared with the same block assembled by hand from
ordinary integrals of shells with l +- 1 (d_m g_l = 2a g_{l+1_m} - l_m g_{l-1_m}, summed over
the primitives of contracted shells).  tests/test_int_cases.py holds an ordinary host integral
to |host - exact| <= kappa(L) 2^-53 sabs (sabs: the same sum over absolute values; kappa from
tests/golden/int_ref.npz).  Both sides here are such sums: the hand-assembled one has the scale
S = sum_terms |coefficient| sabs(term), and the derivative table's own scale is at most S (its
entries are 2a E+ - l E-, so |D| <= 2a |E+| + l |E-| term by term).  Hence
|table - by hand| <= 2 kappa(L) 2^-53 S with L the order of the highest term.  L = 14 takes the
largest stored kappa (see tests/test_gpu_somf.py).
"""
import types

import numpy as np
import pytest

import int_cases as ic

U = 2.0 ** -53
CENTRES = np.array([[0.0, 0.0, 0.0], [0.9, -0.4, 0.3], [-0.5, 0.7, 1.1], [0.2, 1.3, -0.8]])
# as tests/test_gpu_somf.py: every l at every position, the uniform classes, 1 and 3 primitives,
# distinct and coincident centres
CASES = [
    ((0, 0, 0, 0), (3, 1, 1, 3), (0, 1, 2, 3)),
    ((1, 1, 1, 1), (1, 3, 3, 1), (0, 1, 2, 3)),
    ((2, 2, 2, 2), (1, 1, 3, 1), (0, 1, 0, 2)),
    ((3, 3, 3, 3), (1, 1, 1, 1), (0, 1, 2, 3)),
    ((3, 3, 3, 3), (1, 1, 1, 1), (0, 0, 1, 2)),
    ((0, 1, 2, 3), (3, 1, 3, 1), (0, 1, 2, 3)),
    ((1, 2, 3, 0), (1, 3, 1, 3), (0, 1, 2, 3)),
    ((2, 3, 0, 1), (3, 1, 1, 3), (1, 1, 2, 3)),
    ((3, 0, 1, 2), (1, 3, 1, 1), (0, 1, 2, 2)),
    ((0, 0, 0, 3), (1, 1, 3, 3), (0, 0, 1, 1)),
]
IDS = ["".join("spdf"[l] for l in c[0]) + "-n" + "".join(map(str, c[1])) + "-c" + "".join(map(str, c[2])) for c in CASES]


@pytest.fixture(scope="module")
def kappa():
    k = ic.load_fixture()["kappa"]
    return np.concatenate([k, [k.max()] * (15 - len(k))])


def shell(l, nprim, centre, seed):
    from xtddft_amd.qc.gto import Shell, gto_norm
    rng = np.random.default_rng(seed)
    exps = 0.4 * 3.1 ** np.arange(nprim) * (1.0 + 0.3 * rng.random(nprim))
    coefs = (0.5 + rng.random(nprim)) * gto_norm(l, exps)
    return Shell(int(centre), l, CENTRES[centre].copy(), exps, coefs)


def shifted(s):
    """d_m of a contracted shell as a list of (coefficient array over (m, component of s,
    component of the shifted shell), shifted one-primitive shell)."""
    from xtddft_amd.qc.gto import Shell
    from xtddft_amd.qc.ints import cart_comps
    out = []
    comps = cart_comps(s.l)
    for a, c in zip(s.exps, s.coefs):
        for dl in (1, -1):
            if s.l + dl < 0:
                continue
            tgt = cart_comps(s.l + dl)
            pos = {k: i for i, k in enumerate(tgt)}
            w = np.zeros((3, len(comps), len(tgt)))
            for i, comp in enumerate(comps):
                for m in range(3):
                    k = list(comp)
                    k[m] += dl
                    if min(k) >= 0:
                        w[m, i, pos[tuple(k)]] = c * (2.0 * a if dl == 1 else -comp[m])
            out.append((w, Shell(s.atom, s.l + dl, s.center, np.array([a]), np.array([1.0]))))
    return out


def eri_abs(bra, ket):
    """sabs of eri_quartet: the same contraction over absolute values."""
    from xtddft_amd.qc import ints
    p, q = bra.p[:, None], ket.p[None, :]
    d = bra.P[:, None, :] - ket.P[None, :, :]
    R = np.abs(ints.hermite_r(bra.L + ket.L, p * q / (p + q), d[..., 0], d[..., 1], d[..., 2]))
    idx, _ = ints._sum_table(bra.L, ket.L)
    Rm = R[idx] * (2.0 * np.pi ** 2.5 / (p * q * np.sqrt(p + q)))
    X = np.einsum('tsPQ,cdsQ->tcdP', Rm, np.abs(ket.Eab), optimize=True)
    return np.einsum('abtP,tcdP->abcd', np.abs(bra.Eab), X, optimize=True)


def nuc_abs(pair, charges, coords):
    from xtddft_amd.qc import ints
    acc = np.zeros(pair.Eab.shape[:2])
    for z, c in zip(charges, coords):
        d = pair.P - c
        R = np.abs(ints.hermite_r(pair.L, pair.p, d[:, 0], d[:, 1], d[:, 2]))
        acc += abs(z) * np.einsum('abtq,tq->ab', np.abs(pair.Eab), R * (2.0 * np.pi / pair.p))
    return acc


# --------------------------------------------------------------------------- 1: the l-shift identity
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_electron_tables_obey_the_l_shift_identity(kappa, case):
    from xtddft_amd.qc.ints import DerivPair, ShellPair, eri_quartet, somf_quartet
    ls, nps, cs = case
    a, b, c, d = (shell(l, n, ce, 10 * i + l) for i, (l, n, ce) in enumerate(zip(ls, nps, cs)))
    got = somf_quartet(DerivPair(a, b), DerivPair(c, d))                   # (3, ca, cb, cc, cd)
    dd = np.zeros((3, 3) + got.shape[1:])
    scale = np.zeros_like(dd)
    for wa, sa in shifted(a):
        bra = ShellPair(sa, b)
        for wc, sc in shifted(c):
            ket = ShellPair(sc, d)
            dd += np.einsum('mia,nkc,abcd->mnibkd', wa, wc, eri_quartet(bra, ket))
            scale += np.einsum('mia,nkc,abcd->mnibkd', np.abs(wa), np.abs(wc), eri_abs(bra, ket))
    want = np.stack([dd[m, n] - dd[n, m] for m, n in ((1, 2), (2, 0), (0, 1))])
    S = np.stack([scale[m, n] + scale[n, m] for m, n in ((1, 2), (2, 0), (0, 1))])
    L = sum(ls) + 2
    bound = 2.0 * kappa[L] * U * S
    err = np.abs(got - want)
    print(f"(%d%d|%d%d) L={L}: worst |table - by hand| / bound {(err[bound > 0] / bound[bound > 0]).max():.4f}, "
          f"max|K| {np.abs(want).max():.3e}" % ls)
    assert np.any(want != 0.0) and np.all(err <= bound)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_electron_tables_obey_the_l_shift_identity(kappa, case):
    from xtddft_amd.qc.ints import DerivPair, ShellPair
    ls, nps, cs = case
    a, b = (shell(l, n, ce, 10 * i + l) for i, (l, n, ce) in list(enumerate(zip(ls, nps, cs)))[:2])
    charges, coords = np.array([3.0, 1.0, 8.0]), np.array([CENTRES[cs[0]], CENTRES[cs[1]], [0.4, 0.4, -0.6]])
    got = DerivPair(a, b, both=True).nuclear(charges, coords)              # (4, ca, cb)
    dd = np.zeros((3, 3) + got.shape[1:])
    scale = np.zeros_like(dd)
    for wa, sa in shifted(a):
        for wb, sb in shifted(b):
            pair = ShellPair(sa, sb)
            dd += np.einsum('mia,njb,ab->mnij', wa, wb, pair.nuclear(charges, coords))
            scale += np.einsum('mia,njb,ab->mnij', np.abs(wa), np.abs(wb), nuc_abs(pair, charges, coords))
    want = np.stack([dd[0, 0] + dd[1, 1] + dd[2, 2]] + [dd[m, n] - dd[n, m] for m, n in ((1, 2), (2, 0), (0, 1))])
    S = np.stack([scale[0, 0] + scale[1, 1] + scale[2, 2]] + [scale[m, n] + scale[n, m] for m, n in ((1, 2), (2, 0), (0, 1))])
    bound = 2.0 * kappa[ls[0] + ls[1] + 2] * U * S
    err = np.abs(got - want)
    print(f"<%d|V|%d>: worst / bound {(err[bound > 0] / bound[bound > 0]).max():.4f}" % ls[:2])
    assert np.any(want != 0.0) and np.all(err <= bound)


# --------------------------------------------------------------------------- 2: the closed form
def test_closed_form_anchor_and_normalised_wso():
    """x exp(-a r^2), y exp(-b r^2) on a nucleus Z: W^z_xy = -2 pi Z / (3 (a + b)) = -W^z_yx."""
    from xtddft_amd.qc import M
    from xtddft_amd.qc.gto import Shell
    from xtddft_amd.qc.ints import DerivPair
    a, b, Z = 0.7, 1.3, 3.0
    sa, sb = (Shell(0, 1, np.zeros(3), np.array([e]), np.array([1.0])) for e in (a, b))
    w = DerivPair(sa, sb, both=True).nuclear([Z], [np.zeros(3)])
    exact = -2.0 * np.pi * Z / (3.0 * (a + b))
    assert abs(exact - (-3.14159265358979)) < 1e-14
    assert abs(w[3, 0, 1] - exact) < 4 * U * abs(exact) and abs(w[3, 1, 0] + exact) < 4 * U * abs(exact)
    assert abs(w[1, 1, 2] - exact) < 4 * U * abs(exact) and abs(w[2, 2, 0] - exact) < 4 * U * abs(exact)
    # the normalised AOs of a one-atom, p-only basis (Li: Z = 3)
    mol = M("Li 0 0 0", basis={"Li": [[1, [a, 1.0]], [1, [b, 1.0]]]}, spin=1)
    wso = mol.intor("int1e_wso")
    n1 = mol.shells[0].coefs[0] * mol._norm[0]
    n2 = mol.shells[1].coefs[0] * mol._norm[3]
    assert wso.shape == (3, 6, 6)
    assert abs(wso[2, 0, 4] - n1 * n2 * exact) < 1e-14 * abs(exact)        # <d px(1)| V |d py(2)>, z component
    assert abs(wso[2, 1, 3] + n1 * n2 * exact) < 1e-14 * abs(exact)
    assert abs(wso[2, 0, 1] + 2.0 * np.pi * Z / (3.0 * 2 * a) * n1 * n1) < 1e-14 * abs(exact)


# --------------------------------------------------------------------------- 3: symmetries
def test_symmetries_at_rounding():
    from xtddft_amd import somf
    from xtddft_amd.qc import M
    mol = M("F 0 0 0; H 0.2 0.1 0.9", basis="6-31G")
    w = mol._pvp()
    assert np.abs(w[0] - w[0].T).max() < 1e-14 * np.abs(w[0]).max()
    assert np.abs(w[1:] + w[1:].transpose(0, 2, 1)).max() < 1e-14 * np.abs(w[1:]).max()
    assert np.array_equal(w[0], mol.intor("int1e_pnucp")) and np.array_equal(w[1:], mol.intor("int1e_wso_sph"))
    K = somf.kint_host(mol)
    assert np.abs(K + K.transpose(0, 3, 4, 1, 2)).max() < 1e-14 * np.abs(K).max()


# --------------------------------------------------------------------------- 4: X2C algebra
def test_sfx2c1e_identities():
    import scipy.linalg
    from xtddft_amd import somf
    from xtddft_amd.qc import M
    from xtddft_amd.qc.gto import get_xmol
    xmol, cc = get_xmol(M("F 0 0 0; H 0 0 1.0", basis="6-31G"))
    assert cc.shape == (xmol.nao, 11)
    t, v, w, s = (xmol.intor(k) for k in ("int1e_kin", "int1e_nuc", "int1e_pnucp", "int1e_ovlp"))
    assert np.linalg.eigvalsh(s)[0] > 1e-8                       # a primitive appearing twice gives ~1e-16
    c = somf.LIGHT_SPEED
    x, rp, h1e = somf.sfx2c1e(t, v, w, s, c)
    n = s.shape[0]
    h = np.block([[v, t], [t, w * (0.25 / c ** 2) - t]])
    m = np.block([[s, np.zeros((n, n))], [np.zeros((n, n)), t * (0.5 / c ** 2)]])
    e4 = scipy.linalg.eigh(h, m, eigvals_only=True)
    e2 = scipy.linalg.eigh(h1e, s, eigvals_only=True)
    print(f"X2C: max |e(h1e) - e+(Dirac)| {np.abs(e2 - e4[n:]).max():.2e} at |e|max {np.abs(e2).max():.1f}")
    assert np.abs(e2 - e4[n:]).max() < 1e-9 * np.abs(e2).max()
    assert np.abs(h1e - h1e.T).max() < 1e-10
    # the non-relativistic limit: everything within O(c^-2)
    big = 1e6
    x, rp, h1e = somf.sfx2c1e(t, v, w, s, big)
    tol = 100.0 * max(np.abs(w).max(), np.abs(t).max()) ** 2 / big ** 2
    assert np.abs(h1e - (t + v)).max() < tol and np.abs(rp - np.eye(n)).max() < tol and np.abs(x - np.eye(n)).max() < tol


# --------------------------------------------------------------------------- 5: rotation covariance
def test_rotation_covariance_ch2():
    from scipy.spatial.transform import Rotation
    from xtddft_amd import somf
    from xtddft_amd.qc import M
    geom = np.array([[0.0, 0.0, 0.1], [0.0, 0.86, -0.45], [0.3, -0.8, -0.5]])
    R = Rotation.from_rotvec(np.random.default_rng(3).standard_normal(3)).as_matrix()
    assert abs(np.linalg.det(R) - 1.0) < 1e-14

    def mk(x):
        return M([("C", x[0]), ("H", x[1]), ("H", x[2])], basis="6-31G", spin=2)
    m0, m1 = mk(geom), mk(geom @ R.T)
    n = m0.nao
    assert max(s.l for s in m0.shells) == 1
    a = np.random.default_rng(1).standard_normal((n, n))
    dm = a + a.T
    Uao = np.eye(n)
    for s, p0 in zip(m0.shells, m0.ao_loc[:-1]):
        if s.l == 1:
            Uao[p0:p0 + 3, p0:p0 + 3] = R
    none = types.SimpleNamespace()
    v0 = somf.get_soDKH1_somf(none, m0, iop="x2c", include_mf2e=True, use_1c=False, device=None, dm=dm)
    v1 = somf.get_soDKH1_somf(none, m1, iop="x2c", include_mf2e=True, use_1c=False, device=None, dm=Uao @ dm @ Uao.T)
    want = np.einsum('lk,ij,kjm,nm->lin', R, Uao, v0, Uao)
    err = np.abs(v1 - want).max() / np.abs(v0).max()
    print(f"rotation covariance: {err:.2e} of max|Vso| {np.abs(v0).max():.3e}")
    assert err < 1e-10
    assert np.abs(v1 - v0).max() > 1e-3 * np.abs(v0).max()      # the rotation is not a symmetry of the inputs


# --------------------------------------------------------------------------- 6: one-centre
def test_one_centre_approximation():
    from xtddft_amd import somf
    from xtddft_amd.qc import M
    rng = np.random.default_rng(2)
    atom = M("F 0 0 0", basis="6-31G", spin=1)
    n = atom.nao
    p = [rng.standard_normal((n, n)) for _ in range(3)]
    for g1, g0 in zip(somf.somf_g_host(atom, *p, use_1c=True), somf.somf_g_host(atom, *p, use_1c=False)):
        assert np.array_equal(g1, g0)
    mol = M("F 0 0 0; H 0 0 1.0", basis="6-31G")
    n = mol.nao
    p = [rng.standard_normal((n, n)) for _ in range(3)]
    at = mol.ao_atom()
    same = np.ones((n, n, n, n), dtype=bool)
    for ax in range(1, 4):
        same &= np.expand_dims(at, tuple(range(1, 4))) == np.expand_dims(at, tuple(i for i in range(4) if i != ax))
    K = somf.kint_host(mol)
    want = somf.somf_g_host(mol, *p, kint=K * same[None])
    got = somf.somf_g_host(mol, *p, use_1c=True)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() < 1e-13 * np.abs(w).max()
    full = somf.somf_g_host(mol, *p, kint=K)
    assert np.abs(full[0] - want[0]).max() > 1e-3 * np.abs(full[0]).max()


# --------------------------------------------------------------------------- 7: sign of the two-electron term
def test_two_electron_term_screens_the_nuclear_one():
    """O atom, triplet ROKS (HF exchange: the LDA run does not converge for the bare atom) /
    cc-pVDZ, iop 'bp': <px|Vso^z|py> of the tight contracted p shell with the SOMF term keeps the
    sign of the one-electron term and is smaller: 0 < ratio < 1.  Measured 0.659 (Koseki's
    Z_eff / Z for oxygen is about 0.70, recalled, not verifiable here)."""
    from xtddft_amd import somf
    from xtddft_amd.qc import M, ROKS
    mol = M("O 0 0 0", basis="cc-pvdz", spin=2)
    mf = ROKS(mol, "HF")
    mf.kernel()
    assert mf.converged
    shell_p = next(k for k, s in enumerate(mol.shells) if s.l == 1)
    assert mol.shells[shell_p].exps.size == 3
    p0 = mol.ao_loc[shell_p]
    with_2e = somf.get_soDKH1_somf(mf, mol, iop="bp", include_mf2e=True, device=None)
    only_1e = somf.get_soDKH1_somf(mf, mol, iop="bp", include_mf2e=False, device=None)
    ratio = with_2e[2, p0, p0 + 1] / only_1e[2, p0, p0 + 1]
    print(f"O atom: <px|Vso^z|py> with SOMF / without = {ratio:.4f}")
    assert only_1e[2, p0, p0 + 1] != 0.0 and 0.0 < ratio < 1.0
    assert np.abs(with_2e + with_2e.transpose(0, 2, 1)).max() < 1e-15


# --------------------------------------------------------------------------- 8: the sf-X2C mean field
def test_sfx2c1e_scf_n2():
    from xtddft_amd import somf
    from xtddft_amd.qc import M, ROHF
    mol = M("N 0 0 0; N 0 0 1.0977", basis="cc-pvdz")
    plain = ROHF(mol)
    plain.kernel()
    assert not hasattr(plain, "with_x2c")
    assert np.array_equal(plain.get_hcore(), mol.intor("int1e_kin") + mol.intor("int1e_nuc"))   # untouched path
    nr = ROHF(mol).sfx2c1e(1e6)
    nr.kernel()
    rel = ROHF(mol).sfx2c1e()
    rel.kernel()
    assert plain.converged and nr.converged and rel.converged and rel.with_x2c.c == somf.LIGHT_SPEED
    print(f"N2 / cc-pVDZ: E(c = 1e6) - E(nr) = {nr.e_tot - plain.e_tot:.2e} Ha, E(sf-X2C) - E(nr) = {rel.e_tot - plain.e_tot:.6f} Ha")
    assert abs(nr.e_tot - plain.e_tot) < 1e-8
    assert rel.e_tot < plain.e_tot - 1e-3
    xmol, cc = rel.with_x2c.get_xmol(mol)
    assert cc.shape == (xmol.nao, mol.nao) and xmol.nao > mol.nao
    assert np.abs(cc.T @ xmol.intor("int1e_ovlp") @ cc - mol.intor("int1e_ovlp")).max() < 1e-13


def test_vso_mo_and_exports():
    import xtddft_amd
    from xtddft_amd import _capi, build
    v = np.random.default_rng(0).standard_normal((3, 4, 4))
    c = np.random.default_rng(1).standard_normal((4, 4))
    got = xtddft_amd.vso_mo(types.SimpleNamespace(mo_coeff=c), v)
    assert np.abs(got - np.stack([c.T @ x @ c for x in v])).max() < 1e-14
    assert xtddft_amd.get_soDKH1_somf is xtddft_amd.somf.get_soDKH1_somf
    assert "xt_hint_cart" in _capi.EXPORTS and "xt_hint.hip" in build.SOURCES and "xt_hermite.h" in build.HEADERS
    assert _capi.ABI_VERSION == 8
    with pytest.raises(ValueError):
        xtddft_amd.get_soDKH1_somf(types.SimpleNamespace(), xtddft_amd.qc.M("H 0 0 0; H 0 0 0.74", basis="6-31G"), iop="dkh",
                                   device=None, dm=np.zeros((4, 4)))


# --------------------------------------------------------------------------- 9: argument checks
def test_xt_hint_cart_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with its own message before the first HIP
    call -- not XT_ERR_HIP (-3) from a failed one."""
    L = hiplib
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data

    def call(nbra=1, binfo=i, bprim=d, eb=d, nket=1, kinfo=i, kprim=d, ek=d, lbra=3, lket=3, cross=1, nrow_tot=1,
             out=d, ldo=1):
        return L.xt_hint_cart(nbra, binfo, bprim, eb, nket, kinfo, kprim, ek, lbra, lket, cross, nrow_tot, out, ldo, None)

    def rejected(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.xt_last_error(), L.xt_last_error()
    rejected(call(nbra=-1), "negative size")
    rejected(call(nket=-2), "negative size")
    rejected(call(ldo=-1), "negative size")
    rejected(call(lbra=-1), "order")
    rejected(call(lket=-1), "order")
    rejected(call(lbra=9, lket=0), "order")
    rejected(call(lbra=8, lket=7), "order")
    rejected(call(lbra=7, lket=8), "order")
    rejected(call(cross=2), "cross")
    rejected(call(cross=-1), "cross")
    rejected(call(cross=1, nrow_tot=0), "nrow_tot")
    for name in ("binfo", "bprim", "eb", "kinfo", "kprim", "ek", "out"):
        rejected(call(**{name: None}), "null")
    assert call(nbra=0, binfo=None, out=None) == 0 and call(nket=0, kinfo=None) == 0      # nothing to do
