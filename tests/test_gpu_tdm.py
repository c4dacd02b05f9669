"""GPU: state-to-state transition moments (``xt_tdm`` and the ``transition_dipoles`` /
``osc_str`` / ``calculate_TDM`` methods) against the term-by-term restatement of the
reference's formula in tests/tdm_ref.py (XSF_TDA.py:435-592).

The tolerance is the project's RTOL for device-vs-oracle FP64 contractions
(tests/test_gpu_parity.py): max|T_dev - T_ref| / max|T_ref| < 1e-12; the sums here are
shorter than sigma's."""
import ctypes

import numpy as np
import pytest

import tdm_ref
from oracle.xsf_tda import get_vect
from xtddft_amd.synthetic import make_mf

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# ---- raw entry ------------------------------------------------------------------
def make_problem(nc, no, nv, nstates, ncomp, compressed, seed=0, orthonormal=True):
    """Unit-norm random states, a random symmetric AO operator, random square coefficients
    (core | open | virtual columns): dict with both row layouts and the MO operator."""
    rng = np.random.default_rng(seed)
    nao = nc + no + nv
    c = np.linalg.qr(rng.standard_normal((nao, nao)))[0]
    if not orthonormal:   # a well-conditioned non-orthogonal basis: S_AO = C^-T C^-1 != 1
        c = c @ (np.eye(nao) + 0.2 * np.triu(rng.standard_normal((nao, nao)), 1) / np.sqrt(nao))
    op = rng.standard_normal((ncomp, nao, nao))
    op = op + op.transpose(0, 2, 1)
    cv = rng.standard_normal((nstates, nc, nv))
    co = rng.standard_normal((nstates, nc, no))
    ov = rng.standard_normal((nstates, no, nv))
    vects = get_vect(no) if compressed else None
    w = rng.standard_normal((nstates, no * no - (1 if compressed else 0)))
    oo = (w @ vects.T if compressed else w).reshape(nstates, no, no)
    amp = np.concatenate([np.concatenate([co, cv], axis=2), np.concatenate([oo, ov], axis=2)], axis=1)
    norm = np.sqrt((amp ** 2).sum(axis=(1, 2)))
    rows = np.hstack([cv.reshape(nstates, -1), co.reshape(nstates, -1), ov.reshape(nstates, -1), w])
    return dict(nc=nc, no=no, nv=nv, nao=nao, c=c, op=op, vects=vects,
                rows_blocks=np.ascontiguousarray(rows / norm[:, None]),
                rows_ov=np.ascontiguousarray(amp.reshape(nstates, -1) / norm[:, None]))


def reference(p, sa):
    d = np.einsum('xpq,pi,qj->xij', p["op"], p["c"], p["c"])
    return tdm_ref.tdm_roks(p["rows_blocks"], d, p["nc"], p["no"], p["nv"], sa, p["no"] / 2, p["vects"])


def run_tdm(torch, lib, p, sa, layout, device_ptrs, op=None):
    from xtddft_amd import _capi
    nc, no, nv = p["nc"], p["no"], p["nv"]
    op = p["op"] if op is None else op
    vecs = p["rows_ov"] if layout == "ov" else p["rows_blocks"]
    compressed = layout == "blocks" and p["vects"] is not None
    assert layout == "blocks" or p["vects"] is None, "the occ x vir layout has no compressed form"
    arrs = [np.ascontiguousarray(op), np.ascontiguousarray(p["c"][:, :nc + no]),
            np.ascontiguousarray(p["c"][:, nc:]), vecs,
            np.ascontiguousarray(p["vects"]) if compressed else None]   # get_vect returns a strided view
    n, x = vecs.shape[0], op.shape[0]
    d = _capi.XtTdmDesc(nao=p["nao"], nc=nc, no=no, nv=nv, ncomp=x, nstates=n, sa=sa, si=no / 2,
                        layout=_capi.TDM_LAYOUT[layout], oo_compressed=int(compressed))
    if device_ptrs:
        dev = [None if a is None else torch.from_numpy(a).cuda() for a in arrs]
        out = torch.full((x, n, n), float("nan"), dtype=torch.float64, device="cuda")
        ptr = [None if t is None else t.data_ptr() for t in dev]
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(lib.xt_tdm(ctypes.byref(d), *ptr, out.data_ptr(), _capi.XT_PTR_DEVICE, st), "xt_tdm")
        return out.cpu().numpy()
    out = np.full((x, n, n), np.nan)
    ptr = [None if a is None else a.ctypes.data for a in arrs]
    _capi.check(lib.xt_tdm(ctypes.byref(d), *ptr, out.ctypes.data, _capi.XT_PTR_HOST, None), "xt_tdm")
    return out


# (nstates, ncomp, sa, layout, compressed, device pointers): every value of every axis with
# every shape; uncompressed blocks at sa = 3 is the case with f3 and tr(oo) != 0
OPEN_CASES = [(1, 1, 0, "ov", False, False), (7, 3, 3, "blocks", True, True),
              (41, 3, 3, "blocks", False, False), (41, 1, 0, "blocks", True, True),
              (7, 3, 3, "ov", False, True), (1, 3, 0, "blocks", False, True)]
SFUP_CASES = [(1, 1, 0, "ov", False, False), (7, 3, 0, "blocks", False, True),
              (41, 3, 0, "ov", False, True), (41, 1, 0, "blocks", False, False)]
RAW = ([(s, c) for s in [(3, 2, 5), (5, 3, 18), (17, 2, 33), (1, 2, 1)] for c in OPEN_CASES]
       + [((6, 0, 9), c) for c in SFUP_CASES])


@pytest.mark.parametrize("shape,case", RAW)
def test_xt_tdm_matches_the_restatement(torch, hiplib, shape, case):
    nstates, ncomp, sa, layout, compressed, device_ptrs = case
    p = make_problem(*shape, nstates, ncomp, compressed, seed=nstates + ncomp)
    ref = reference(p, sa)
    t = run_tdm(torch, hiplib, p, sa, layout, device_ptrs)
    err = np.abs(t - ref).max() / np.abs(ref).max()
    print(f"shape {shape} case {case}: rel err {err:.2e}")
    assert err < RTOL


@pytest.mark.parametrize("sa,compressed", [(0, False), (3, False), (3, True)])
def test_xt_tdm_is_symmetric_and_deterministic(torch, hiplib, sa, compressed):
    p = make_problem(5, 3, 18, 7, 3, compressed, seed=11)
    t = run_tdm(torch, hiplib, p, sa, "blocks", True)
    asym = np.abs(t - t.transpose(0, 2, 1)).max() / np.abs(t).max()
    print(f"sa {sa} compressed {compressed}: asymmetry {asym:.2e}")
    assert asym < 1e-13
    assert np.array_equal(t, run_tdm(torch, hiplib, p, sa, "blocks", True))
    assert np.array_equal(t, run_tdm(torch, hiplib, p, sa, "blocks", False))


@pytest.mark.parametrize("sa", [0, 3])
def test_xt_tdm_vanishes_for_the_overlap(torch, hiplib, sa):
    """An operator c S_AO (S_AO = C^-T C^-1) has no moments, diagonal ones included: the
    origin of the dipole operator does not matter."""
    p = make_problem(5, 3, 18, 7, 3, False, seed=12, orthonormal=False)
    cinv = np.linalg.inv(p["c"])
    coef = np.array([0.7, -1.3, 2.1])
    t = run_tdm(torch, hiplib, p, sa, "blocks", True, op=coef[:, None, None] * (cinv.T @ cinv))
    worst = (np.abs(t).max(axis=(1, 2)) / np.abs(coef)).max()
    print(f"sa {sa}: max|T| / |c| = {worst:.2e}")
    assert worst < 1e-12


def test_xt_tdm_chunked_states_match(torch, hiplib, monkeypatch):
    """A workspace budget of 48 KiB makes 41 states of (5,3,18) run in chunks of 6."""
    p = make_problem(5, 3, 18, 41, 3, True, seed=13)
    ref = reference(p, 3)
    whole = run_tdm(torch, hiplib, p, 3, "blocks", True)
    monkeypatch.setenv("XT_TDM_WS_MIB", "0.047")
    for device_ptrs in (True, False):
        t = run_tdm(torch, hiplib, p, 3, "blocks", device_ptrs)
        assert np.abs(t - ref).max() / np.abs(ref).max() < RTOL
        assert np.abs(t - whole).max() / np.abs(ref).max() < 1e-13
    q = make_problem(6, 0, 9, 41, 1, False, seed=14)
    t = run_tdm(torch, hiplib, q, 0, "ov", True)
    assert np.abs(t - reference(q, 0)).max() / np.abs(reference(q, 0)).max() < RTOL


# ---- drivers -----------------------------------------------------------------------
def sym_operator(nao, seed=21):
    op = np.random.default_rng(seed).standard_normal((3, nao, nao))
    return op + op.transpose(0, 2, 1)


def check_driver(x, ref_of):
    """transition_dipoles / osc_str of a solved driver against the restatement on the same
    eigenpairs."""
    op = sym_operator(x.mf.nao)
    t = x.transition_dipoles(op_ao=op)
    ref = ref_of(op)
    n = ref.shape[1]
    assert t.shape == (3, n, n)
    err = np.abs(t - ref).max() / np.abs(ref).max()
    print(f"{type(x).__name__}: rel err {err:.2e}")
    assert err < RTOL
    o, oref = x.osc_str(op_ao=op), tdm_ref.osc(np.asarray(x.e)[:n], ref)
    assert o.shape == (n, n)
    assert np.abs(o - oref).max() / np.abs(oref).max() < RTOL


@pytest.mark.parametrize("sa", [0, 3])
def test_xsf_roks_transition_dipoles(torch, sa):
    from xtddft_amd import XSF_TDA
    mf = make_mf(nao=28, nc=5, no=3, xctype="GGA", hyb=0.5)
    x = XSF_TDA(mf, SA=sa)
    x.kernel(nstates=6)
    assert x.re and np.asarray(x.v).shape[1] >= 6

    def ref_of(op):
        d = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff, mf.mo_coeff)
        return tdm_ref.tdm_roks(np.asarray(x.v).T, d, x.nc, x.no, x.nv, sa, mf.mol.spin / 2, x.vects)
    check_driver(x, ref_of)


def test_xsf_uks_transition_dipoles(torch):
    from xtddft_amd import XSF_TDA
    mf = make_mf(nao=28, nc=5, no=3, xctype="GGA", hyb=0.5, kind="U")
    x = XSF_TDA(mf)
    x.kernel(nstates=6)
    nc, no = x.nc, x.no

    def ref_of(op):
        aa = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff[0], mf.mo_coeff[0])
        bb = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff[1], mf.mo_coeff[1])
        return tdm_ref.tdm_uks(np.asarray(x.v).T, aa[:, :nc + no, :nc + no], bb[:, nc:, nc:], nc, no, x.nv,
                               x.vects if x.re else None)
    check_driver(x, ref_of)


@pytest.mark.parametrize("isf", [-1, 1])
def test_sf_tda_transition_dipoles(torch, isf):
    from xtddft_amd.sf_tda import SF_TDA
    mf = make_mf(nao=28, nc=5, no=3, xctype="GGA", hyb=0.5)
    x = SF_TDA(mf, isf=isf)
    x.kernel(nstates=5)
    nc, no, nv = x.nc, x.no, x.nv
    vecs = np.asarray(x.v)[:, :5].T

    def ref_of(op):
        d = np.einsum('xpq,pi,qj->xij', op, mf.mo_coeff, mf.mo_coeff)
        if isf == -1:   # alpha occupied -> beta virtual, cv|co|ov|oo rows
            return tdm_ref.tdm_uks(vecs, d[:, :nc + no, :nc + no], d[:, nc:, nc:], nc, no, nv)
        # beta occupied (nc) -> alpha virtual (nv): one cv block
        return tdm_ref.tdm_uks(vecs, d[:, :nc, :nc], d[:, nc + no:, nc + no:], nc, 0, nv)
    check_driver(x, ref_of)


def test_hf_molecule_dipoles_do_not_depend_on_the_origin(torch, capsys):
    """HF / 6-31G triplet ROKS (the XSF parity molecule): the default operator is int1e_r at
    the centre of nuclear charge; the same roots with the origin at 0 give the same moments,
    and calculate_TDM prints the reference's table, one line per ordered pair."""
    from molecules import hf_meanfield
    from xtddft_amd import XSF_TDA
    mf = hf_meanfield("ROKS")
    x = XSF_TDA(mf)
    x.kernel(nstates=4)
    capsys.readouterr()
    t, o = x.calculate_TDM(verbose=True)
    lines = capsys.readouterr().out.strip().split("\n")
    n = np.asarray(x.v).shape[1]
    assert n >= 4 and t.shape == (3, n, n) and o.shape == (n, n)
    assert lines[1].startswith("State State") and len(lines) == 2 + n * n
    t0 = x.transition_dipoles(op_ao=mf.extra["qc_mol"].intor_symmetric("int1e_r", comp=3))
    print(f"origin shift: max |dT| = {np.abs(t - t0).max():.2e}, max|T| = {np.abs(t).max():.3f}")
    assert np.abs(t).max() > 1e-3
    assert np.abs(t - t0).max() < 1e-10
    d = np.einsum('xpq,pi,qj->xij', mf.extra["qc_mol"].intor_symmetric("int1e_r", comp=3),
                  mf.mo_coeff, mf.mo_coeff)
    ref = tdm_ref.tdm_roks(np.asarray(x.v).T, d, x.nc, x.no, x.nv, x.SA, mf.mol.spin / 2, x.vects)
    assert np.abs(t0 - ref).max() < RTOL * max(1.0, np.abs(ref).max())
