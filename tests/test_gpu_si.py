"""GPU: the spin-orbit state-interaction couplings (``xt_si_couple``) and the driver
``xtddft_amd.soc.SI_driver`` against the restatement of si_driver.py / tdm.py in
tests/si_ref.py, the exactly solvable limits through the device route, and the pinned
``xt_tdm_sc`` path.

Tolerances: device against restatement element-wise 1e-12 of the largest element (the
project's bar for FP64 contractions, tests/test_gpu_tdm_sc.py); spin-orbit levels
1e-12 ||H_eff|| (the perturbation bound of a Hermitian eigenproblem for that element error
is ||dH|| <= n max|dH_ij|, far below it at these n); the limits 1e-12 at O(1) magnitudes."""
import ctypes
import types

import numpy as np
import pytest

import si_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# (nc, no, nv), S, states (S-, So, S+)
SHAPES = [((3, 2, 4), 1.0, (4, 5, 3)), ((2, 1, 3), 0.5, (0, 4, 3)), ((2, 0, 3), 0.0, (0, 3, 4)),
          ((5, 3, 7), 1.5, (6, 5, 4))]
BIG = ((37, 2, 70), 1.0, (9, 11, 7))


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def rows(states, n):
    return [ref.rows_of(states, k, d) for k, d in zip(('|S->', '|So>', '|S+>'), ref.dims(*n))]


def fake_mf(nc, no, nv):
    """What SI_driver reads of a mean field: the Mole's counts (no integrals, MO basis = AO basis)."""
    from xtddft_amd import Mole
    nmo = nc + no + nv
    return types.SimpleNamespace(mol=Mole(nao=nmo, spin=no, nelectron=2 * nc + no), e_tot=0.0, mo_coeff=np.eye(nmo))


_PROBLEMS = {}


def problem(shape, s, counts, seed=0):
    """Inputs and both restatement results, computed once per shape and left unchanged."""
    key = (shape, s, counts, seed)
    if key not in _PROBLEMS:
        vso, dip, states = ref.random_problem(*shape, counts, seed=seed)
        xs = rows(states, shape)
        want = {"soc": ref.couple(vso, s, *shape, *xs, True, "soc"), "dipole": ref.couple(dip, s, *shape, *xs, True, "dipole")}
        for a in (vso, dip, *xs, *want.values()):
            a.setflags(write=False)
        _PROBLEMS[key] = dict(vso=vso, dip=dip, states=states, xs=xs, want=want)
    return _PROBLEMS[key]


def rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("mode", ["soc", "dipole"])
@pytest.mark.parametrize("shape,s,counts", SHAPES)
def test_couplings_match_the_restatement(torch, shape, s, counts, mode):
    from xtddft_amd.soc import si_couple
    p = problem(shape, s, counts)
    got = si_couple(p["vso"] if mode == "soc" else p["dip"], s, *shape, *p["xs"], with_ground=True, mode=mode)
    want = p["want"][mode]
    assert got.shape == want.shape
    err = rel(got, want)
    print(f"{shape} S={s} {mode}: rel err {err:.2e}, max|T| {np.abs(want).max():.3f}")
    assert err < RTOL
    # the blocks that stay zero: below the diagonal, S-/S+ and GS/GS; for the moments all but same S
    g = np.repeat(np.arange(4), (counts[0], 1, counts[1], counts[2]))
    gl, gr = np.meshgrid(g, g, indexing="ij")
    if mode == "soc":
        zero = (gl > gr) | ((gl == 0) & (gr == 3)) | ((gl == 1) & (gr == 1))
    else:
        zero = ~(((gl == gr) & (gl != 1)) | ((gl == 1) & (gr == 2)))
    assert np.all(got[:, zero] == 0.0) and np.all(want[:, zero] == 0.0)


@pytest.mark.parametrize("mode", ["soc", "dipole"])
def test_device_pointers_and_identical_bits(torch, hiplib, mode):
    """Device pointers give the bits of host pointers, and two calls the same bits."""
    from xtddft_amd import _capi
    from xtddft_amd.soc import si_couple
    shape, s, counts = SHAPES[3]
    p = problem(shape, s, counts)
    op = p["vso"] if mode == "soc" else p["dip"]
    a = si_couple(op, s, *shape, *p["xs"], mode=mode)
    assert np.array_equal(a, si_couple(op, s, *shape, *p["xs"], mode=mode))
    n = a.shape[1]
    d = _capi.XtSiDesc(nc=shape[0], no=shape[1], nv=shape[2], ncomp=3, s=s, n_sm=counts[0], n_so=counts[1],
                       n_sp=counts[2], with_ground=1, mode=_capi.SI_MODE[mode])
    dev = [torch.from_numpy(np.array(x)).cuda() for x in (op, *p["xs"])]      # copies: the shared inputs are read-only
    out = torch.full((3, n, n), float("nan"), dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(hiplib.xt_si_couple(ctypes.byref(d), *[t.data_ptr() for t in dev], out.data_ptr(),
                                    _capi.XT_PTR_DEVICE, st), "xt_si_couple")
    assert np.array_equal(a, out.cpu().numpy())


def test_chunked_states_match(torch, monkeypatch):
    """(37, 2, 70) with a 0.5 MiB budget: 2 states per chunk, so every pair of manifolds runs
    several right-hand and left-hand chunks, the last one short."""
    from xtddft_amd.soc import si_couple
    shape, s, counts = BIG
    p = problem(shape, s, counts, seed=3)
    whole = {m: si_couple(p["vso"] if m == "soc" else p["dip"], s, *shape, *p["xs"], mode=m) for m in ("soc", "dipole")}
    monkeypatch.setenv("XT_TDM_WS_MIB", "0.5")
    for m in ("soc", "dipole"):
        got = si_couple(p["vso"] if m == "soc" else p["dip"], s, *shape, *p["xs"], mode=m)
        err, split = rel(got, p["want"][m]), rel(got, whole[m])
        print(f"{m}: chunked vs restatement {err:.2e}, whole vs restatement {rel(whole[m], p['want'][m]):.2e}, "
              f"chunked vs whole {split:.2e}")
        assert err < RTOL and rel(whole[m], p["want"][m]) < RTOL


@pytest.mark.parametrize("drop", ["|S->", "|So>", "|S+>", "ngs"])
def test_empty_groups(torch, drop):
    from xtddft_amd.soc import si_couple
    shape, s, counts = SHAPES[0]
    p = problem(shape, s, counts)
    xs = [x if k != drop else x[:0] for k, x in zip(('|S->', '|So>', '|S+>'), p["xs"])]
    g = drop != "ngs"
    for mode, op in (("soc", p["vso"]), ("dipole", p["dip"])):
        want = ref.couple(op, s, *shape, *xs, g, mode)
        got = si_couple(op, s, *shape, *xs, with_ground=g, mode=mode)
        assert got.shape == want.shape
        assert rel(got, want) < RTOL


def driver(shape, s, vso, states, ngs=1, **kw):
    from xtddft_amd.soc import SI_driver
    return SI_driver(fake_mf(*shape), s, vso, ngs=ngs, states=states, **kw)


@pytest.mark.parametrize("shape,s,counts", SHAPES + [BIG])
def test_levels_match_the_restatement(torch, shape, s, counts):
    p = problem(shape, s, counts, seed=3 if (shape, s, counts) == BIG else 0)
    d = driver(shape, s, p["vso"], p["states"])
    eso, vso = d.kernel(printnum=0)
    h, hso, omega = ref.heff(p["vso"], s, *shape, p["states"], 1)
    norm = np.linalg.norm(h, 2)
    print(f"{shape} S={s}: max|dH| {np.abs(d.heff - h).max():.2e}, max|dE| {np.abs(eso - np.linalg.eigvalsh(h)).max():.2e}, "
          f"||H|| {norm:.3f}")
    assert np.abs(d.heff - h).max() < RTOL * np.abs(h).max()
    assert np.abs(d.hso - hso).max() < RTOL * np.abs(h).max() and np.array_equal(d.Omega, omega)
    assert np.abs(eso - np.linalg.eigvalsh(h)).max() < RTOL * norm
    assert np.abs(vso.conj().T @ d.heff @ vso - np.diag(eso)).max() < 1e-11 * norm


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_exact_limits_on_the_device(torch, name):
    lim = ref.limit(name, 1 if name == "d" else 2)
    d = driver((lim["nc"], lim["no"], lim["nv"]), lim["S"], lim["vso"], lim["states"])
    eso, _ = d.kernel(printnum=0)
    err = np.abs(eso - lim["exact"]).max()
    print(f"limit ({name}): worst difference {err:.2e}")
    assert eso.shape == lim["exact"].shape and err < 1e-12
    if lim["S"] == 0.5:
        assert np.abs(eso[0::2] - eso[1::2]).max() < 1e-12     # Kramers pairs


def test_dipole_blocks_equal_the_pinned_xt_tdm_sc(torch):
    """The So/So and GS/So blocks of XT_SI_DIPOLE equal ``transition_moments_sc(...,
    spin_adapted=True)`` for the same roots taken through ``states_from_xtda``: this fixes
    the CV(1) sign of the helper (xt_tdm_sc carries -g in so2st's phase, tdm.py +g)."""
    from xtddft_amd import tdm
    from xtddft_amd.soc import si_couple, states_from_xtda
    from xtddft_amd.utils import order_pyscf2my
    nc, no, nv = 5, 3, 7
    nmo = nc + no + nv
    rng = np.random.default_rng(7)
    vecs = np.linalg.qr(rng.standard_normal(((nc + no) * nv + nc * (no + nv), 6)))[0].T
    a = rng.standard_normal((3, nmo, nmo))
    dip = a + a.transpose(0, 2, 1)
    c = np.eye(nmo)
    want = tdm.transition_moments_sc(dip, c[:, :nc + no], c[:, nc + no:], c[:, :nc], c[:, nc:], vecs,
                                     spin_adapted=True, no=no, si=no / 2, ground=True)
    x = types.SimpleNamespace(X=True, nc=nc, no=no, nv=nv, v=vecs.T[order_pyscf2my(nc, no, nv), :], e=np.arange(6.0))
    states = states_from_xtda(x)
    xso = np.array([s[1] for s in states])
    got = si_couple(dip, no / 2, nc, no, nv, None, xso, None, with_ground=True, mode="dipole")
    scale = np.abs(want).max()
    print(f"So/So {np.abs(got[:, 1:, 1:] - want[:, 1:, 1:]).max() / scale:.2e}, "
          f"GS/So {np.abs(got[:, 0, 1:] - want[:, 0, 1:]).max() / scale:.2e}")
    assert np.abs(got[:, 1:, 1:] - want[:, 1:, 1:]).max() < RTOL * scale
    assert np.abs(got[:, 0, 1:] - want[:, 0, 1:]).max() < RTOL * scale
    flipped = xso.copy()
    flipped[:, -nc * nv:] *= -1.0                                  # so2st's own CV(1) phase does not pass
    bad = si_couple(dip, no / 2, nc, no, nv, None, flipped, None, with_ground=True, mode="dipole")
    assert np.abs(bad[:, 1:, 1:] - want[:, 1:, 1:]).max() > 1e-3 * scale


def test_triplet_molecule_end_to_end(torch, capsys):
    """HF / 6-31G triplet ROKS: XSF, X-TDA and SF-up roots through the three helpers into
    SI_driver with a seeded Vso of magnitude 1e-3."""
    from molecules import hf_meanfield
    from xtddft_amd import SF_TDA, SI_driver, XSF_TDA, XTDA, states_from_sf_up, states_from_xsf, states_from_xtda
    mf = hf_meanfield("ROKS")
    xsf = XSF_TDA(mf)
    xsf.kernel(nstates=4)
    xt = XTDA(mf.mol, mf, nstates=4)
    xt.kernel()
    up = SF_TDA(mf, isf=1)
    up.kernel(nstates=3)
    states = {'|S->': states_from_xsf(xsf), '|So>': states_from_xtda(xt), '|S+>': states_from_sf_up(up)}
    nc, no, nv = xt.nc, xt.no, xt.nv
    assert no == 2 and [len(states[k]) for k in ('|S->', '|So>', '|S+>')] == [4, 4, 3]
    dsm, dso, dsp = ref.dims(nc, no, nv)
    assert all(x.shape == (dsm,) for _, x in states['|S->']) and all(x.shape == (dso,) for _, x in states['|So>'])
    assert all(x.shape == (dsp,) for _, x in states['|S+>'])
    o12 = nc * nv + nc * no + no * nv
    for _, x in states['|S->']:                                     # O1O2 has a zero diagonal; the norm survives
        assert np.all(x[o12 + np.arange(no) * (no + 1)] == 0.0) and abs(x @ x - 1.0) < 1e-8
    nmo = nc + no + nv
    a = np.random.default_rng(11).standard_normal((3, nmo, nmo))
    vso = 1e-3 * (a - a.transpose(0, 2, 1))
    si = SI_driver(mf, 1.0, vso, ngs=1, states=states, cal_osc=True)
    eso, v = si.kernel(printnum=5)
    out = capsys.readouterr().out
    assert "Interaction among 4 |S-⟩, 1 |GS⟩, 4 |So⟩, 3 |S+⟩." in out
    dim = 1 * 4 + 3 * (1 + 4) + 5 * 3
    assert si.heff.shape == (dim, dim) and eso.shape == (dim,)
    h, _, _ = ref.heff(vso, 1.0, nc, no, nv, states, 1)
    print(f"molecule: max|dH| {np.abs(si.heff - h).max():.2e}, max|hso| {np.abs(si.hso).max():.2e}")
    assert np.abs(si.hso).max() > 1e-5
    assert np.abs(si.heff - h).max() < RTOL * np.abs(h).max()
    assert np.abs(eso - np.linalg.eigvalsh(h)).max() < RTOL * np.linalg.norm(h, 2)
    # esf and the labels: a weak Vso leaves every level with a dominant parent whose energy is esf
    for i in range(dim):
        label, e_sf = si.v2state(v[:, i])
        pos = int(np.argmax((v[:, i].conj() * v[:, i]).real))
        S, M, ith, igs = si.cal_pos(pos)
        assert e_sf == si.states[si.S2str[(S, igs)]][ith][0] == si.Omega[pos, pos]
        assert f"{ith:>3d}-th" in label and f"{M:+.1f}" in label
    assert np.abs(si.esf - np.einsum('ij,i,ij->j', v.conj(), np.diag(si.Omega), v).real).max() < 1e-14
    # h_so has a zero diagonal: the levels and their spin-free parents share the trace of Omega
    assert abs(eso.sum() - np.trace(si.Omega)) < 1e-11 and abs(si.esf.sum() - np.trace(si.Omega)) < 1e-11
    assert np.abs(si.esf - eso).max() < 0.05                        # a 1e-3 coupling moves no level far
    assert si.dm.shape == (dim, dim, 3) and si.dmso.shape == (dim, dim, 3)
    for x in range(3):
        assert np.abs(si.dmso[..., x] - si.dmso[..., x].conj().T).max() < 1e-12 * max(1.0, np.abs(si.dm).max())
    dE, f = si.print_osc_local(0, dim - 1)
    assert dE == eso[dim - 1] - eso[0] and np.isfinite(f)
