"""CPU: the state-interaction restatement (tests/si_ref.py) in its exactly solvable limits and
symmetries, the host side of ``xtddft_amd.soc`` run on that restatement, and the host side of
``xt_si_couple`` (declaration, export, descriptor layout, argument validation before any HIP
call)."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import si_ref as ref
from xtddft_amd import Mole, soc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xtddft_amd.h")

# (nc, no, nv), S, states (S-, So, S+)
SHAPES = [((3, 2, 4), 1.0, (4, 5, 3)), ((2, 1, 3), 0.5, (0, 4, 3)), ((2, 0, 3), 0.0, (0, 3, 4)),
          ((5, 3, 7), 1.5, (6, 5, 4))]


def fake_mf(nc, no, nv, spin=None):
    nmo = nc + no + nv
    return types.SimpleNamespace(mol=Mole(nao=nmo, spin=no if spin is None else spin, nelectron=2 * nc + no),
                                 e_tot=0.0, mo_coeff=np.eye(nmo))


def driver(shape, s, vso, states, ngs=1, **kw):
    """SI_driver with the restatement in the place of the device call."""
    d = soc.SI_driver(fake_mf(*shape), s, vso, ngs=ngs, states=states, **kw)
    d.couple = ref.couple
    return d


# ---- the four exact limits ---------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_exact_limit(name):
    """Eigenvalues of H_eff = eigenvalues of H_so + diag(energies) projected on the explicit spin
    eigenfunctions.  Worst differences when written: (a) 9e-16, (b) 3e-15, (c) 2e-15, (d) 8e-15."""
    lim = ref.limit(name, 1 if name == "d" else 2)
    shape = (lim["nc"], lim["no"], lim["nv"])
    h, _, _ = ref.heff(lim["vso"], lim["S"], *shape, lim["states"], 1)
    err = np.abs(np.linalg.eigvalsh(h) - lim["exact"]).max()
    print(f"limit ({name}) restatement: {err:.2e}")
    assert err < 1e-12
    d = driver(shape, lim["S"], lim["vso"], lim["states"])
    eso, _ = d.kernel(printnum=0)
    assert np.abs(d.heff - h).max() < 1e-13
    assert np.abs(eso - lim["exact"]).max() < 1e-12
    if name in "ab":                                            # every level doubly degenerate
        assert np.abs(eso[0::2] - eso[1::2]).max() < 1e-12


def test_limit_d_needs_the_normalised_antisymmetric_o1o1_vector():
    """With (1, 1)/sqrt 2 or another norm in O1O1 the triplet limit fails: the check has teeth."""
    lim = ref.limit("d", 1)
    shape = (lim["nc"], lim["no"], lim["nv"])
    for vec in (np.array([1.0, 1.0]) / np.sqrt(2), np.array([1.0, -1.0])):
        states = {k: list(v) for k, v in lim["states"].items()}
        e, x = states['|S->'][-1]
        x = x.copy()
        x[-2:] = vec
        states['|S->'][-1] = (e, x)
        h, _, _ = ref.heff(lim["vso"], lim["S"], *shape, states, 1)
        assert np.abs(np.linalg.eigvalsh(h) - lim["exact"]).max() > 1e-3


# ---- Wigner-Eckart factor ----------------------------------------------------------------
def test_closed_form_w_against_sympy():
    pytest.importorskip("sympy")
    n = 0
    for S in (0, 0.5, 1, 1.5, 2):
        for Sp in (S - 1, S, S + 1):
            if Sp < 0:
                continue
            for M in np.arange(-S, S + 1):
                for Mp in np.arange(-Sp, Sp + 1):
                    assert abs(soc.w(S, M, Sp, Mp) - ref.w_sympy(S, M, Sp, Mp)) < 1e-14, (S, M, Sp, Mp)
                    n += 1
    assert n == 4 + 12 + 27 + 48 + 75                     # (2S+1)(2S'+1) summed over the allowed S'
    assert soc.w(0, 0, 0, 0) == 0.0                       # the reference's vanishing denominator
    with pytest.raises(ValueError):
        soc.w(1, 0.5, 1, 0)
    with pytest.raises(ValueError):
        soc.w(0.3, 0, 1, 0)


def test_soc_module_does_not_import_sympy():
    out = subprocess.check_output([sys.executable, "-c",
                                   "import sys; import xtddft_amd.soc as s; s.w(1, 0, 1, 1); print('sympy' in sys.modules)"],
                                  cwd=ROOT, text=True)
    assert out.strip() == "False"


# ---- symmetries of the restatement ----------------------------------------------------------
@pytest.mark.parametrize("shape,s,counts", SHAPES)
def test_same_manifold_blocks_are_hermitian(shape, s, counts):
    """h^m is i times a real antisymmetric combination, so <L||h||R> of one manifold is
    anti-Hermitian-by-component in the way that makes H_eff Hermitian: the blocks filled in full
    must agree with their own Hermitian completion.  Ties the twice-written case pairs 2, 3,
    13, 14, 21, 22, 29, 48, 49, 50, 54, 57 to each other."""
    vso, dip, states = ref.random_problem(*shape, counts, seed=1)
    xs = [ref.rows_of(states, k, d) for k, d in zip(('|S->', '|So>', '|S+>'), ref.dims(*shape))]
    c = ref.couple(vso, s, *shape, *xs, True, "soc")
    scale = np.abs(c).max()
    first = np.cumsum([0, counts[0], 1, counts[1], counts[2]])
    for g in (g for g in (0, 2, 3) if first[g + 1] > first[g]):
        blk = c[:, first[g]:first[g + 1], first[g]:first[g + 1]]
        # real antisymmetric operator: the real couplings are antisymmetric under L <-> R
        assert np.abs(blk + blk.transpose(0, 2, 1)).max() < 1e-12 * scale
    t = ref.couple(dip, s, *shape, *xs, True, "dipole")
    for g in (g for g in (0, 2, 3) if first[g + 1] > first[g]):
        blk = t[:, first[g]:first[g + 1], first[g]:first[g + 1]]
        assert np.abs(blk - blk.transpose(0, 2, 1)).max() < 1e-12 * np.abs(t).max()
    # and H_eff before completion: fill both triangles of a same-manifold block from the full block
    hm = np.einsum('mk,kij->mij', soc.HM, c)
    for g, S_g in ((0, s - 1), (2, s), (3, s + 1)):
        if first[g + 1] == first[g] or S_g < 0:
            continue
        blk = hm[:, first[g]:first[g + 1], first[g]:first[g + 1]]
        for M in np.arange(-S_g, S_g + 1):
            for Mp in np.arange(-S_g, S_g + 1):
                if abs(M - Mp) > 1:
                    continue
                a = blk[int(Mp - M) + 1] * soc.w(S_g, M, S_g, Mp)
                b = blk[int(M - Mp) + 1] * soc.w(S_g, Mp, S_g, M)
                assert np.abs(a - b.conj().T).max() < 1e-12 * scale


@pytest.mark.parametrize("shape,s,counts", [SHAPES[1], SHAPES[3]])
def test_kramers_pairs(shape, s, counts):
    vso, _, states = ref.random_problem(*shape, counts, seed=2)
    eso, _ = driver(shape, s, vso, states).kernel(printnum=0)
    assert eso.size % 2 == 0
    assert np.abs(eso[0::2] - eso[1::2]).max() < 1e-12 * np.abs(eso).max()


@pytest.mark.parametrize("shape,s,counts", SHAPES)
def test_levels_are_invariant_under_rotations_of_vso(shape, s, counts):
    vso, _, states = ref.random_problem(*shape, counts, seed=3)
    q = np.linalg.qr(np.random.default_rng(4).standard_normal((3, 3)))[0]
    q *= np.sign(np.linalg.det(q))                              # proper rotation
    e0, _ = driver(shape, s, vso, states).kernel(printnum=0)
    e1, _ = driver(shape, s, np.einsum('kl,lpq->kpq', q, vso), states).kernel(printnum=0)
    assert np.abs(e1 - e0).max() < 1e-12 * np.abs(e0).max()
    assert np.abs(e0 - np.sort(np.diag(driver(shape, s, 0 * vso, states).make_heff()).real)).max() > 1e-3


@pytest.mark.parametrize("shape,s,counts", SHAPES)
def test_zero_vso_returns_omega_with_multiplicities(shape, s, counts):
    vso, _, states = ref.random_problem(*shape, counts, seed=5)
    d = driver(shape, s, 0.0 * vso, states)
    eso, _ = d.kernel(printnum=0)
    want = [0.0] * int(2 * s + 1)
    for key, spin in (('|S->', s - 1), ('|So>', s), ('|S+>', s + 1)):
        for e, _ in states[key]:
            want += [e] * int(2 * spin + 1)
    assert np.array_equal(eso, np.sort(want)) and np.all(d.hso == 0.0)
    assert d.dim_hso == len(want)


@pytest.mark.parametrize("shape,s,counts", SHAPES + [((3, 2, 4), 1.0, (0, 5, 0))])
@pytest.mark.parametrize("ngs", [0, 1])
def test_cal_pos_inverts_cal_hso_pos(shape, s, counts, ngs):
    vso, _, states = ref.random_problem(*shape, counts, seed=6)
    d = driver(shape, s, vso, states, ngs=ngs)
    seen = set()
    for p in range(d.dim_hso):
        S, M, ith, igs = d.cal_pos(p)
        assert d.cal_hso_pos(S, M, ith, igs, S, M, ith, igs) == (p, p)
        assert -S <= M <= S and (igs == 1) == (d.S2str[(S, igs)] == '|GS>')
        seen.add((S, M, ith, igs))
    assert len(seen) == d.dim_hso
    # position = group offset + M_index n_group + i
    if counts[1]:
        assert d.cal_hso_pos(s, -s + 1 if s else 0.0, 2, 0, s, -s, 0, 0) == \
            (d.dim1 + (1 if s else 0) * counts[1] + 2, d.dim1)
    with pytest.raises(ValueError):
        d.cal_pos(d.dim_hso)


def test_driver_matches_the_reference_assembly_and_moments():
    shape, s, counts = SHAPES[0]
    vso, dip, states = ref.random_problem(*shape, counts, seed=7)
    mu = np.array([0.1, -0.2, 0.3])
    d = driver(shape, s, vso, states, cal_osc=True, dipole_ao=dip, ref_dipole=mu)
    eso, v = d.kernel(printnum=0)
    h, hso, omega = ref.heff(vso, s, *shape, states, 1)
    assert np.abs(d.heff - h).max() < 1e-13 and np.abs(d.hso - hso).max() < 1e-13 and np.array_equal(d.Omega, omega)
    assert np.all(np.diag(d.hso) == 0.0)
    assert np.abs(d.esf - np.diag(v.conj().T @ omega @ v).real).max() < 1e-13
    xs = [ref.rows_of(states, k, n) for k, n in zip(('|S->', '|So>', '|S+>'), ref.dims(*shape))]
    t = ref.couple(dip, s, *shape, *xs, True, "dipole")
    # same (S, M) blocks, the reference moment on the diagonal
    p, q = d.cal_hso_pos(s, 0.0, 1, 0, s, 0.0, 3, 0)
    assert np.abs(d.dm[p, q] - t[:, counts[0] + 1 + 1, counts[0] + 1 + 3]).max() < 1e-14
    assert np.abs(d.dm[q, p] - d.dm[p, q]).max() == 0.0
    p, q = d.cal_hso_pos(s, 1.0, 0, 1, s, 1.0, 2, 0)
    assert np.abs(d.dm[p, q] - t[:, counts[0], counts[0] + 1 + 2]).max() < 1e-14
    p, q = d.cal_hso_pos(s, 1.0, 0, 1, s, 0.0, 2, 0)
    assert np.all(d.dm[p, q] == 0.0)
    p, _ = d.cal_hso_pos(s + 1, -2.0, 1, 0, s + 1, -2.0, 1, 0)
    assert np.abs(d.dm[p, p] - (t[:, -counts[2] + 1, -counts[2] + 1] + mu)).max() < 1e-14
    for x in range(3):
        assert np.abs(d.dmso[..., x] - v.conj().T @ d.dm[..., x] @ v).max() < 1e-13
        assert np.abs(d.dmso[..., x] - d.dmso[..., x].conj().T).max() < 1e-13
    with pytest.raises(ValueError, match="cal_osc"):
        driver(shape, s, vso, states).print_osc_local(0, 1)


# ---- ValueError paths ---------------------------------------------------------------------
def test_driver_value_errors():
    shape, s, counts = SHAPES[0]
    vso, _, states = ref.random_problem(*shape, counts, seed=8)
    nmo = sum(shape)
    with pytest.raises(ValueError, match="mol.spin"):
        soc.SI_driver(fake_mf(*shape), 0.5, vso, states=states)
    with pytest.raises(ValueError, match="Vso"):
        driver(shape, s, vso[:2], states)
    with pytest.raises(ValueError, match="Vso"):
        driver(shape, s, np.zeros((3, nmo + 1, nmo + 1)), states)
    with pytest.raises(ValueError, match="antisymmetric"):
        driver(shape, s, vso + np.eye(nmo), states)
    with pytest.raises(ValueError, match="antisymmetric"):
        driver(shape, s, np.abs(vso), states)
    bad = dict(states)
    bad['|So>'] = [(0.1, states['|So>'][0][1][:-1])]
    with pytest.raises(ValueError, match="length"):
        driver(shape, s, vso, bad)
    bad = dict(states)
    bad['|So>'] = [(0.1, states['|So>'][0][1][:shape[0] * shape[2] + shape[0] * shape[1] + shape[1] * shape[2]])]
    with pytest.raises(ValueError, match="length"):                 # S > 0: the CV(1) block is not optional
        driver(shape, s, vso, bad)
    with pytest.raises(ValueError, match="labels"):
        driver(shape, s, vso, {'|S0>': []})
    # |S-> states below S = 1
    shape2, s2, counts2 = SHAPES[1]
    vso2, _, st2 = ref.random_problem(*shape2, counts2, seed=8)
    st2['|S->'] = [(0.2, np.zeros(ref.dims(*shape2)[0]))]
    with pytest.raises(ValueError, match="S >= 1"):
        driver(shape2, s2, vso2, st2)
    # S = 0: a |So> vector without its CV(1) block is padded
    shape0, s0, counts0 = SHAPES[2]
    vso0, _, st0 = ref.random_problem(*shape0, counts0, seed=8)
    short = {k: list(v) for k, v in st0.items()}
    short['|So>'] = [(e, x[:shape0[0] * shape0[2]]) for e, x in st0['|So>']]
    e_full, _ = driver(shape0, s0, vso0, st0).kernel(printnum=0)
    e_short, _ = driver(shape0, s0, vso0, short).kernel(printnum=0)
    assert np.array_equal(e_full, e_short)


def test_helpers_reject_the_wrong_solver():
    with pytest.raises(ValueError):
        soc.states_from_xtda(types.SimpleNamespace(X=False))
    with pytest.raises(ValueError):
        soc.states_from_sf_up(types.SimpleNamespace(isf=-1))


def test_states_from_xsf_splits_the_open_block():
    nc, no, nv, n = 2, 3, 2, 4
    rng = np.random.default_rng(9)
    d3 = nc * nv + nc * no + no * nv
    vects = np.linalg.qr(rng.standard_normal((no * no, no * no - 1)))[0]
    v = rng.standard_normal((d3 + no * no - 1, n))
    x = types.SimpleNamespace(nc=nc, no=no, nv=nv, v=v, vects=vects, re=True, e=np.arange(n) + 0.5)
    states = soc.states_from_xsf(x)
    assert [e for e, _ in states] == [0.5, 1.5, 2.5, 3.5]
    for i, (_, s) in enumerate(states):
        oo = (vects @ v[d3:, i]).reshape(no, no)
        assert s.shape == (d3 + no * no + no,) and np.array_equal(s[:d3], v[:d3, i])
        assert np.allclose(s[d3:d3 + no * no].reshape(no, no), oo - np.diag(np.diag(oo)), rtol=0, atol=1e-15)
        assert np.allclose(s[d3 + no * no:], np.diag(oo), rtol=0, atol=1e-15)
    x.re, x.v = False, rng.standard_normal((d3 + no * no, n))
    s = soc.states_from_xsf(x)[1][1]
    assert np.array_equal(s[d3 + no * no:], np.diag(x.v[d3:, 1].reshape(no, no)))


def test_package_reexports():
    import xtddft_amd
    for name in ("SI_driver", "si_couple", "states_from_xsf", "states_from_xtda", "states_from_sf_up"):
        assert getattr(xtddft_amd, name) is getattr(soc, name) and name in xtddft_amd.__all__


# ---- the entry's host side ---------------------------------------------------------------------
def test_header_declares_and_library_exports_xt_si_couple(hiplib):
    txt = open(HEADER).read()
    assert re.search(r"^\s*int\s+xt_si_couple\s*\(", txt, re.M)
    assert "#define XT_SI_SOC 0" in txt and "#define XT_SI_DIPOLE 1" in txt
    assert "XT_ABI_VERSION 8" in txt                          # a pure addition: no bump
    assert hasattr(hiplib, "xt_si_couple")
    from xtddft_amd import _capi, build
    assert "xt_si_couple" in _capi.EXPORTS and "xt_si.hip" in build.SOURCES
    assert _capi.ABI_VERSION == 8 and _capi.SI_MODE == {"soc": 0, "dipole": 1}


def test_si_desc_layout_matches_c_header(tmp_path):
    from xtddft_amd._capi import XtSiDesc
    fields = [f for f, _ in XtSiDesc._fields_]
    assert set(fields) == {"nc", "no", "nv", "ncomp", "s", "n_sm", "n_so", "n_sp", "with_ground", "mode"}
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xtddft_amd.h"\nint main(){'
                   'printf("%zu", sizeof(xt_si_desc));' +
                   "".join(f'printf(" %zu", offsetof(xt_si_desc, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(XtSiDesc)
    assert out[1:] == [getattr(XtSiDesc, f).offset for f in fields]


def test_xt_si_couple_rejects_bad_arguments_without_gpu(hiplib):
    """Every validation case returns XT_ERR_ARG (-1) with a message before any HIP call."""
    from xtddft_amd import _capi
    nc, no, nv = 3, 2, 4
    nmo = nc + no + nv
    dsm, dso, dsp = ref.dims(nc, no, nv)
    op = np.zeros((3, nmo, nmo))
    xs = dict(sm=np.zeros((4, dsm)), so=np.zeros((5, dso)), sp=np.zeros((3, dsp)))
    out = np.zeros((3, 13, 13))

    def call(null=None, desc=True, ptr_kind=_capi.XT_PTR_HOST, **kw):
        f = dict(nc=nc, no=no, nv=nv, ncomp=3, s=1.0, n_sm=4, n_so=5, n_sp=3, with_ground=1, mode=0)
        f.update(kw)
        d = _capi.XtSiDesc(**f)
        ptrs = dict(op=op, sm=xs["sm"], so=xs["so"], sp=xs["sp"], out=out)
        args = [None if k == null else a.ctypes.data for k, a in ptrs.items()]
        rc = hiplib.xt_si_couple(ctypes.byref(d) if desc else None, *args, ptr_kind, None)
        return rc, hiplib.xt_last_error()

    rc, msg = call(desc=False)
    assert rc == -1 and b"descriptor" in msg
    for k in ("op", "sm", "so", "sp", "out"):
        rc, msg = call(null=k)
        assert rc == -1 and b"null" in msg, k
    for kw in (dict(nc=-1), dict(no=-1, s=-0.5), dict(nv=-1), dict(nc=0, no=0, nv=0, s=0.0, n_sm=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"orbital counts" in msg, kw
    for k in ("n_sm", "n_so", "n_sp"):
        rc, msg = call(**{k: -1})
        assert rc == -1 and b"state counts" in msg, k
    rc, msg = call(n_sm=0, n_so=0, n_sp=0, with_ground=0)
    assert rc == -1 and b"state counts" in msg
    rc, msg = call(ncomp=0)
    assert rc == -1 and b"ncomp" in msg
    rc, msg = call(mode=2)
    assert rc == -1 and b"mode" in msg
    rc, msg = call(with_ground=2)
    assert rc == -1 and b"with_ground" in msg
    for s in (0.5, 1.5, -1.0, float("nan")):
        rc, msg = call(s=s)
        assert rc == -1 and b"no / 2" in msg, s
    rc, msg = call(no=1, s=0.5)                                # |S-> below S = 1
    assert rc == -1 and b"S >= 1" in msg
    with pytest.raises(ValueError, match="S >= 1"):
        _capi.check(rc, "xt_si_couple")
    rc, msg = call(nc=1 << 20, nv=1 << 20)
    assert rc == -1 and b"2^21" in msg
    rc, msg = call(nc=2000, nv=2000)                           # nmo fits, the vectors do not
    assert rc == -1 and b"dim >= 2^21" in msg
    rc, msg = call(nv=0, n_so=0, n_sm=0)                       # |S+> states of an empty manifold
    assert rc == -1 and b"empty manifold" in msg
    rc, msg = call(ptr_kind=2)
    assert rc == -1 and b"ptr_kind" in msg
    # an empty group may come with a null pointer -- then only ptr_kind is left to refuse
    rc, msg = call(null="sm", n_sm=0, ptr_kind=7)
    assert rc == -1 and b"ptr_kind" in msg


def test_si_couple_checks_shapes_before_the_library():
    with pytest.raises(ValueError, match="operator"):
        soc.si_couple(np.zeros((3, 5, 5)), 1.0, 3, 2, 4)
    with pytest.raises(ValueError, match=r"\|So> vectors"):
        soc.si_couple(np.zeros((3, 9, 9)), 1.0, 3, 2, 4, x_so=np.zeros((2, 7)))
