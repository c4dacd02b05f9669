"""GPU: transition moments between spin-conserving roots (``xt_tdm_sc`` and the ``XTDA``
methods ``transition_dipoles`` / ``osc_matrix`` / ``state_dipoles`` / ``calculate_TDM``) against
the term-by-term restatement of TDM_S / TDM_GSS in tests/xtda_tdm_ref.py
(x2c_hamiltonian/driver/tdm.py:6-126, xtddft/XTDA.py:1354-1400).

The tolerance is the project's RTOL for device-vs-oracle FP64 contractions
(tests/test_gpu_parity.py, tests/test_gpu_tdm.py): max|T_dev - T_ref| / max|T_ref| < 1e-12."""
import ctypes

import numpy as np
import pytest

import xtda_tdm_ref as ref
from xtddft_amd.synthetic import make_mf

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# ---- raw entry ------------------------------------------------------------------
def basis(rng, nao):
    """A well-conditioned non-orthogonal square coefficient matrix: S_AO = C^-T C^-1 != 1."""
    c = np.linalg.qr(rng.standard_normal((nao, nao)))[0]
    return c @ (np.eye(nao) + 0.2 * np.triu(rng.standard_normal((nao, nao)), 1) / np.sqrt(nao))


def make_problem(shape, nstates, ncomp, seed=0):
    """Random unit-norm states in PySCF order, a random symmetric AO operator, random
    non-orthogonal coefficients.  ``shape`` (nc, no, nv): one ROKS coefficient matrix
    [c|o|v], spin-adapted with S = no/2; ``shape`` (nocc_a, nvir_a, nocc_b, nvir_b): UKS
    with different C_a, C_b, spin-orbital."""
    rng = np.random.default_rng(seed)
    if len(shape) == 3:
        nc, no, nv = shape
        counts = (nc + no, nv, nc, no + nv)
        ca = cb = basis(rng, nc + no + nv)
    else:
        counts = shape
        nc = no = nv = None
        assert shape[0] + shape[1] == shape[2] + shape[3]
        ca, cb = basis(rng, shape[0] + shape[1]), basis(rng, shape[0] + shape[1])
    oa, va, ob, vb = counts
    nao = ca.shape[0]
    op = rng.standard_normal((ncomp, nao, nao))
    op = op + op.transpose(0, 2, 1)
    vecs = rng.standard_normal((nstates, oa * va + ob * vb))
    vecs /= np.sqrt((vecs ** 2).sum(axis=1))[:, None]
    return dict(counts=counts, roks=(nc, no, nv), sa=len(shape) == 3, nao=nao, ca=ca, cb=cb, op=op,
                vecs=np.ascontiguousarray(vecs))


def reference(p, ground, op=None):
    op = p["op"] if op is None else op
    oa, va, ob, vb = p["counts"]
    if p["sa"]:
        nc, no, nv = p["roks"]
        d = np.einsum('xpq,pi,qj->xij', op, p["ca"], p["ca"])
        return ref.tdm_xtda(p["vecs"], d, nc, no, nv, no / 2, ground=bool(ground))
    daa = np.einsum('xpq,pi,qj->xij', op, p["ca"], p["ca"])
    dbb = np.einsum('xpq,pi,qj->xij', op, p["cb"], p["cb"])
    return ref.tdm_so(p["vecs"], daa, dbb, oa, va, ob, vb, ground=bool(ground))


def run_sc(torch, lib, p, ground, device_ptrs, op=None):
    from xtddft_amd import _capi
    oa, va, ob, vb = p["counts"]
    op = p["op"] if op is None else op
    no = p["roks"][1] if p["sa"] else 0
    arrs = [np.ascontiguousarray(op), np.ascontiguousarray(p["ca"][:, :oa]), np.ascontiguousarray(p["ca"][:, oa:]),
            np.ascontiguousarray(p["cb"][:, :ob]), np.ascontiguousarray(p["cb"][:, ob:]), p["vecs"]]
    n, x = p["vecs"].shape[0], op.shape[0]
    d = _capi.XtTdmScDesc(nao=p["nao"], nocc_a=oa, nvir_a=va, nocc_b=ob, nvir_b=vb, ncomp=x, nstates=n,
                          spin_adapted=int(p["sa"]), no=no, si=no / 2, with_ground=int(ground))
    n1 = n + int(ground)
    if device_ptrs:
        dev = [torch.from_numpy(a).cuda() for a in arrs]
        out = torch.full((x, n1, n1), float("nan"), dtype=torch.float64, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(lib.xt_tdm_sc(ctypes.byref(d), *[t.data_ptr() for t in dev], out.data_ptr(),
                                  _capi.XT_PTR_DEVICE, st), "xt_tdm_sc")
        return out.cpu().numpy()
    out = np.full((x, n1, n1), np.nan)
    _capi.check(lib.xt_tdm_sc(ctypes.byref(d), *[a.ctypes.data for a in arrs], out.ctypes.data,
                              _capi.XT_PTR_HOST, None), "xt_tdm_sc")
    return out


# (nstates, ncomp, with_ground, device pointers): every value of every axis at every shape
CASES = [(1, 1, 0, False), (7, 3, 1, True), (41, 3, 0, True), (41, 1, 1, False), (1, 3, 1, True), (7, 1, 0, False)]
SHAPES = [(3, 2, 5), (5, 3, 18), (17, 2, 33), (1, 1, 1), (6, 0, 9), (8, 20, 5, 23)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_xt_tdm_sc_matches_the_restatement(torch, hiplib, shape, case):
    nstates, ncomp, ground, device_ptrs = case
    p = make_problem(shape, nstates, ncomp, seed=nstates + ncomp)
    want = reference(p, ground)
    t = run_sc(torch, hiplib, p, ground, device_ptrs)
    assert t.shape == want.shape
    err = np.abs(t - want).max() / np.abs(want).max()
    print(f"shape {shape} case {case}: rel err {err:.2e}")
    assert err < RTOL


@pytest.mark.parametrize("device_ptrs", [True, False])
def test_xt_tdm_sc_empty_beta_block(torch, hiplib, device_ptrs):
    """No beta electrons (nocc_b = 0): the beta block is empty and launches nothing."""
    p = make_problem((3, 6, 0, 9), 7, 3, seed=9)
    want = reference(p, 1)
    t = run_sc(torch, hiplib, p, 1, device_ptrs)
    assert np.abs(t - want).max() / np.abs(want).max() < RTOL


@pytest.mark.parametrize("shape", [(5, 3, 18), (8, 20, 5, 23)])
def test_xt_tdm_sc_is_symmetric_and_deterministic(torch, hiplib, shape):
    p = make_problem(shape, 7, 3, seed=11)
    t = run_sc(torch, hiplib, p, 1, True)
    asym = np.abs(t - t.transpose(0, 2, 1)).max() / np.abs(t).max()
    print(f"shape {shape}: asymmetry {asym:.2e}")
    assert asym < 1e-13
    assert np.array_equal(t, run_sc(torch, hiplib, p, 1, True))
    assert np.array_equal(t, run_sc(torch, hiplib, p, 1, False))
    assert np.array_equal(run_sc(torch, hiplib, p, 1, False), run_sc(torch, hiplib, p, 1, False))


@pytest.mark.parametrize("shape", [(5, 3, 18), (8, 20, 5, 23)])
def test_xt_tdm_sc_vanishes_for_the_overlap(torch, hiplib, shape):
    """An operator c S_AO (S_AO = C^-T C^-1) has no moments, ground row and diagonal included:
    the origin of the dipole operator does not matter.  (For the UKS shape S_AO is that of
    C_a and C_b = C_a U with U orthogonal: both spins span one AO metric.)"""
    p = make_problem(shape, 7, 3, seed=12)
    if not p["sa"]:
        u = np.linalg.qr(np.random.default_rng(5).standard_normal((p["nao"], p["nao"])))[0]
        p["cb"] = p["ca"] @ u
    cinv = np.linalg.inv(p["ca"])
    coef = np.array([0.7, -1.3, 2.1])
    t = run_sc(torch, hiplib, p, 1, True, op=coef[:, None, None] * (cinv.T @ cinv))
    worst = (np.abs(t).max(axis=(1, 2)) / np.abs(coef)).max()
    print(f"shape {shape}: max|T| / |c| = {worst:.2e}")
    assert worst < 1e-12


def test_xt_tdm_sc_chunked_states_match(torch, hiplib, monkeypatch):
    """A workspace budget of 0.05 MiB makes 41 states of (5,3,18) run in chunks of 4."""
    p = make_problem((5, 3, 18), 41, 3, seed=13)
    want = reference(p, 1)
    whole = run_sc(torch, hiplib, p, 1, True)
    monkeypatch.setenv("XT_TDM_WS_MIB", "0.05")
    for device_ptrs in (True, False):
        t = run_sc(torch, hiplib, p, 1, device_ptrs)
        assert np.abs(t - want).max() / np.abs(want).max() < RTOL
        assert np.abs(t - whole).max() / np.abs(want).max() < 1e-13


# ---- drivers -----------------------------------------------------------------------
def sym_operator(nao, seed=21):
    op = np.random.default_rng(seed).standard_normal((3, nao, nao))
    return op + op.transpose(0, 2, 1)


def pyscf_rows(x):
    """The solved roots as rows in PySCF order [za | zb] (x.v is in "my order")."""
    return np.ascontiguousarray(np.asarray(x.v)[np.argsort(x.order), :].T)


@pytest.mark.parametrize("davidson", [True, False])
@pytest.mark.parametrize("kind", ["RO", "U"])
def test_xtda_transition_dipoles(torch, kind, davidson):
    from xtddft_amd import XTDA
    mf = make_mf(nao=28, nc=5, no=3, xctype="GGA", hyb=0.5, kind=kind)
    x = XTDA(None, mf, nstates=6, use_Davidson=davidson)
    x.kernel()
    n = np.asarray(x.v).shape[1]
    assert n == 6
    nc, no, nv = x.nc, x.no, x.nv
    op = sym_operator(mf.nao)
    vecs = pyscf_rows(x)
    if kind == "RO":
        d = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff, mf.mo_coeff)
        want = ref.tdm_xtda(vecs, d, nc, no, nv, no / 2)
    else:
        daa = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff[0], mf.mo_coeff[0])
        dbb = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff[1], mf.mo_coeff[1])
        want = ref.tdm_so(vecs, daa, dbb, nc + no, nv, nc, no + nv)
    t = x.transition_dipoles(op_ao=op)
    assert t.shape == (3, n + 1, n + 1)
    err = np.abs(t - want).max() / np.abs(want).max()
    print(f"{kind} davidson={davidson}: rel err {err:.2e}")
    assert err < RTOL
    tx = x.transition_dipoles(op_ao=op, ground=False)
    assert tx.shape == (3, n, n)
    assert np.abs(tx - want[:, 1:, 1:]).max() / np.abs(want[:, 1:, 1:]).max() < RTOL
    e = np.concatenate([[0.0], np.asarray(x.e)[:n]])
    o, oref = x.osc_matrix(op_ao=op), ref.osc(e, want)
    assert o.shape == (n + 1, n + 1)
    assert np.abs(o - oref).max() / np.abs(oref).max() < RTOL
    # the tie to the host path the project pins against the reference's printed f values
    f = x.osc_str(dipole_ao=op)
    tie = np.abs(o[0, 1:] - f).max() / np.abs(f).max()
    print(f"{kind} davidson={davidson}: osc_matrix row 0 vs osc_str {tie:.2e}")
    assert tie < 1e-12


def test_hf_molecule_moments(torch, capsys):
    """HF / 6-31G triplet ROKS (S = 1), 4 roots: the default operator is int1e_r at the centre
    of nuclear charge; the same roots with the origin at 0 give the same moments;
    calculate_TDM prints the reference's two tables; state_dipoles adds the reference moment."""
    from molecules import hf_meanfield
    from xtddft_amd import XTDA
    mf = hf_meanfield("ROKS")
    x = XTDA(mf.mol, mf, nstates=4)
    x.kernel()
    n = np.asarray(x.v).shape[1]
    assert n == 4
    capsys.readouterr()
    t, o = x.calculate_TDM(verbose=True)
    lines = capsys.readouterr().out.rstrip("\n").split("\n")
    assert t.shape == (3, n + 1, n + 1) and o.shape == (n + 1, n + 1)
    assert lines[0] == "Ground state to Excited state transition dipole moments(a.u.)"
    assert len(lines[:n + 1]) == 1 + n and all("|GS⟩" in s for s in lines[1:n + 1])
    assert lines[n + 1] == ""
    assert lines[n + 2] == "Excited state to Excited state transition dipole moments(a.u.)"
    assert lines[n + 3] == "StateL StateR      X        Y        Z      f(L<-R)"
    assert len(lines) == (1 + n) + 1 + 2 + n * n
    r_ao = mf.extra["qc_mol"].intor_symmetric("int1e_r", comp=3)
    t0 = x.transition_dipoles(op_ao=r_ao)
    print(f"origin shift: max |dT| = {np.abs(t - t0).max():.2e}, max|T| = {np.abs(t).max():.3f}")
    assert np.abs(t).max() > 1e-3
    assert np.abs(t - t0).max() < 1e-10
    d = np.einsum('xpq,pi,qj->xij', r_ao, mf.mo_coeff, mf.mo_coeff)
    want = ref.tdm_xtda(pyscf_rows(x), d, x.nc, x.no, x.nv, x.no / 2)
    assert x.no == 2
    assert np.abs(t0 - want).max() < RTOL * max(1.0, np.abs(want).max())
    assert np.abs(o - ref.osc(np.concatenate([[0.0], np.asarray(x.e)[:n]]), t)).max() < 1e-12
    gs = np.array([0.1, -0.2, 0.7])
    sd = x.state_dipoles(reference=gs)
    assert sd.shape == (n, 3)
    assert np.abs(sd - (np.einsum('xii->ix', t[:, 1:, 1:]) + gs)).max() < 1e-12
    assert np.abs(x.state_dipoles() - np.einsum('xii->ix', t[:, 1:, 1:])).max() < 1e-12
