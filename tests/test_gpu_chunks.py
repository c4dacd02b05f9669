"""GPU: the chunked loops of the operator context (xt_ctx_jk.hip over the auxiliary index,
xt_ctx_xc.hip over the grid) against the oracle.

xt_apply and its setters walk the grid and the auxiliary (DF) index in chunks whose sizes
follow from fixed byte budgets (8 GiB for the XC buffers, 1 GiB for the AO -> MO grid
transform, 2 GiB per df_to_mo staging buffer, 3 GiB for the exchange intermediates of
sandwich and exchange_main).  At test sizes every budget holds the whole problem, so a
chunk offset g0 > 0 or p0 > 0, a ragged last chunk and the beta = (p0 == 0 ? 0 : 1) switch
of the sandwich never run.  A wrong offset still gives a symmetric, linear operator: only
a comparison with the oracle sees it.

The test hook XT_CHUNK_BYTES (environment, read once at xt_create) caps every one of
these budgets.  All cases here (but test_chunk_floors) run with XT_CHUNK_BYTES = 65536 and
compare sigma with the oracle's vind on the same make_mf data at the suite's tolerance (1e-12 relative max-norm,
RTOL of test_gpu_parity.py; ERI8_TOL for the stored-ERI case).

`plan()` restates the chunk rules of xt_ctx_jk.hip and xt_ctx_xc.hip (budget = min(default,
XT_CHUNK_BYTES), chunk_budget in xt_ctx.h; project_ao and grid_chunk for the grid; the
floors of one aux row, one grid row and 64 XC points).  Every test asserts from it that the
loops it means to exercise take at least 3 chunks with a ragged last one, so a change of
the shapes or of the rule cannot turn a case into a single-chunk run unnoticed.  With five
trial vectors that holds for every loop a case runs; a single vector leaves some
intermediates inside 64 KiB (the LDA / one-channel XC buffers, the one-group exchange),
so the one-vector cases assert the loops that still split.

Base shape: nao = 26, nc = 5, no = 2 (XSF: no = 3), naux = 78, ngrid = 1000:
  grid transform   315 rows: 315, 315, 315, 55
  df_to_mo         12 aux rows: 6 x 12 + 6
  exchange_main    5 aux rows at nz = 5 (X-TDA: 15 x 5 + 3), 27 at nz = 1
  xc_response      81 points (GGA X-TDA, nz = 5), 64 (MGGA: the floor), 163 (one channel)
  sandwich         XSF SA = 3, nz = 5: 30 aux rows in the largest left-branch (ov_cv_k) and
                   right-branch (cv_ov_k) products: 30, 30, 18
"""
import functools
import os

import numpy as np
import pytest

from oracle import sf_tda as osf
from oracle import xsf_tda as oxsf
from oracle import xtda as oxtda
from xtddft_amd.synthetic import as_eri8, make_mf, make_trial_vectors

pytestmark = pytest.mark.gpu
RTOL = 1e-12
ERI8_TOL = 1e-11        # as in test_gpu_parity.py
CHUNK_BYTES = 65536


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture
def env():
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# ---- the chunk rules of xt_ctx_jk.hip / xt_ctx_xc.hip, restated -------------------------
def _split(total, size):
    """(chunk length, number of chunks, length of the last chunk)"""
    n = -(-total // size)
    return size, n, total - (n - 1) * size


def _split_ok(s):
    size, n, last = s
    return n >= 3 and last != size


def plan(mf, kind, nz, *, nc, no, sf_kernel="alda0", naux=None, ngrid=None, budget=CHUNK_BYTES):
    """Chunking of every budgeted loop for this operator: name -> (size, count, last)."""
    nao = mf.nao
    nv = nao - nc - no
    naux = mf.naux if naux is None else naux
    ngrid = mf.grids.ngrid if (ngrid is None and mf.xctype != "HF") else (ngrid or 0)
    sf = kind in ("SF_DOWN", "SF_UP", "XSF")
    if kind == "SF_UP":
        O, V, nch = nc, nv, 1
    else:
        O, V, nch = nc + no, no + nv, 1 if sf else 2
    groups = [nch * nz] if (sf or mf.is_rohf) else [nz, nz]      # vectors per channel group
    dens_only = sf and sf_kernel == "alda0"
    gga = mf.xctype in ("GGA", "MGGA") and not dens_only
    mgga = mf.xctype == "MGGA" and not dens_only
    out = {}
    if ngrid:
        out["grid"] = _split(ngrid, max(1, min(budget // (8 * nao), ngrid)))
        per_g = nch * nz * O * (4 if mgga else 1) + (nch * nz * 3 if gga else 0)
        G = min(budget // (8 * per_g), ngrid)
        if G < 64:
            G = min(64, ngrid)
        out["xc"] = _split(ngrid, G)
    out["df"] = _split(naux, min(max(1, budget // (8 * nao * nao)), naux))
    for q, nzg in enumerate(groups):
        out[f"exchange{q}"] = _split(naux, min(max(1, budget // (8 * O * nzg * V)), naux))
    if kind == "XSF":
        # the Delta-A exchange products of xsf_delta_a (SA >= 2, and oo sources / targets for
        # SA = 3): (nry, nrx, ncx, ncy) = rows of the left factor, columns of it, rows of the
        # right factor, columns of it
        c, o, v = nc, no, nv
        calls = dict(cv_co=(c, c, o, v), co_cv=(c, c, v, o), cv_ov=(c, o, v, v), ov_cv=(o, c, v, v),
                     co_ov=(c, o, v, o), ov_co=(o, c, o, v), cv_oo=(c, o, o, v), oo_cv=(o, c, v, o),
                     co_oo=(c, o, o, o), oo_co=(o, c, o, o), ov_oo=(o, o, o, v), oo_ov=(o, o, v, o))
        for name, (nry, nrx, ncx, ncy) in calls.items():
            left = 2.0 * nry * nrx * nz * ncx + 2.0 * nry * nz * ncx * ncy
            right = 2.0 * nz * nrx * ncx * ncy + 2.0 * nry * nrx * nz * ncy
            per = nry * nz * ncx if left <= right else nz * nrx * ncy
            side = "left" if left <= right else "right"
            out[f"sandwich_{side}_{name}"] = _split(naux, min(max(1, budget // (8 * per)), naux))
    return out


def assert_chunked(p, names):
    """Every loop in `names` (prefix match) takes >= 3 chunks and a ragged last one."""
    for want in names:
        hit = [k for k in p if k.startswith(want)]
        assert hit, (want, sorted(p))
        if want.startswith("sandwich"):      # at least one product of that branch
            assert any(_split_ok(p[k]) for k in hit), {k: p[k] for k in hit}
        else:
            assert all(_split_ok(p[k]) for k in hit), {k: p[k] for k in hit}


def _has_k(mf):
    return mf.xctype == "HF" or mf.hyb != 0 or mf.omega != 0


def loops_meant(p, mf, nz, k_mode, extra=()):
    """The loops a case asserts: grid and df_to_mo always; with five vectors also the XC loop
    and (direct exchange) exchange_main; with one vector those of them that still split."""
    names = ["df"] + (["grid"] if "grid" in p else [])
    cand = (["xc"] if "xc" in p else []) + (["exchange"] if (k_mode == "direct" and _has_k(mf)) else [])
    for c in cand:
        if nz >= 5 or all(_split_ok(p[k]) for k in p if k.startswith(c)):
            names.append(c)
    return names + list(extra)


# ---- shared references: one mean field and one oracle operator per case -----------------
@functools.lru_cache(maxsize=None)
def _xtda_case(xct, rsh, kind, nao=26, nc=5, no=2, ngrid=1000):
    kw = dict(omega=0.33, alpha=0.65, hyb=0.19) if rsh else dict(hyb=0.2)
    mf = make_mf(nao=nao, nc=nc, no=no, ngrid=ngrid, xctype=xct, kind=kind, **kw)
    vind, hdiag = oxtda.gen_tda_operation(mf)
    return mf, vind, hdiag.size


@functools.lru_cache(maxsize=None)
def _sf_case(xct, kind, isf, method):
    mf = make_mf(nao=26, nc=5, no=2, ngrid=1000, xctype=xct, kind=kind, hyb=0.5)
    vind, hdiag = osf.gen_tda_operation_sf(mf, isf, method=method)
    return mf, vind, hdiag.size


@functools.lru_cache(maxsize=None)
def _xsf_case(method):
    mf = make_mf(nao=26, nc=5, no=3, ngrid=1000, xctype="GGA", hyb=0.5)
    o = oxsf.XSFOracle(mf, SA=3, method=method)
    fg = oxsf.default_fglobal(mf)
    vind, hdiag = o.gen_tda_operation_sf(foo=0.7, fglobal=fg)
    return mf, o, fg, vind, hdiag.size


_REFS = {}


def _reference(case, nz):
    """(trial vectors, oracle sigma) of a cached case, computed once and left unchanged."""
    key = (id(case), nz)        # the case tuples live in the caches above
    if key not in _REFS:
        vind, dim = case[-2], case[-1]
        z = make_trial_vectors(nz, dim)
        ref = vind(z)
        z.setflags(write=False)
        ref.setflags(write=False)
        _REFS[key] = (z, ref)
    return _REFS[key]


def _check(op, z, ref, tol=RTOL):
    r = rel(op.apply(z), ref)
    print(f"rel = {r:.3e}")
    assert r < tol


# ---- base shape ------------------------------------------------------------------------
@pytest.mark.parametrize("k_mode", ["direct", "stored"])
@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("xct,rsh", [("LDA", False), ("GGA", False), ("MGGA", False), ("HF", False), ("GGA", True)])
def test_xtda_chunked(hiplib, env, xct, rsh, nz, k_mode):
    """X-TDA on ROKS; the range-separated case sends a second factor through df_to_mo and
    a second pass through exchange_main."""
    from xtddft_amd.operator import DeviceOperator
    case = _xtda_case(xct, rsh, "RO")
    mf = case[0]
    p = plan(mf, "XTDA", nz, nc=5, no=2)
    assert_chunked(p, loops_meant(p, mf, nz, k_mode))
    if xct != "HF":
        assert p["grid"] == (315, 4, 55)
    assert p["df"] == (12, 7, 6)
    if (xct, nz) == ("GGA", 5):
        assert p["xc"][0] == 81
    if (xct, nz) == ("MGGA", 5):
        assert p["xc"][0] == 64
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    op = DeviceOperator(mf, "XTDA", k_mode=k_mode)
    assert op.k_mode == k_mode
    _check(op, *_reference(case, nz))


@pytest.mark.parametrize("k_mode", ["direct", "stored"])
@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("xct", ["LDA", "GGA", "MGGA"])
def test_utda_chunked(hiplib, env, xct, nz, k_mode):
    """U-TDA on UKS: two MO bases through the grid transform and df_to_mo, two channel
    groups (two exchange loops, two U / wv blocks per XC chunk)."""
    from xtddft_amd.operator import DeviceOperator
    case = _xtda_case(xct, False, "U")
    mf = case[0]
    p = plan(mf, "UTDA", nz, nc=5, no=2)
    assert "exchange1" in p
    assert_chunked(p, loops_meant(p, mf, nz, k_mode))
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    op = DeviceOperator(mf, "UTDA", k_mode=k_mode)
    assert op.k_mode == k_mode
    _check(op, *_reference(case, nz))


@pytest.mark.parametrize("k_mode", ["direct", "stored"])
@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("xct,kind,sf_kernel", [("GGA", "RO", "alda0"), ("GGA", "U", "alda0"), ("LDA", "RO", "mc"),
                                                ("GGA", "RO", "mc"), ("MGGA", "RO", "mc")])
@pytest.mark.parametrize("isf", [-1, 1])
def test_sf_chunked(hiplib, env, isf, xct, kind, sf_kernel, nz, k_mode):
    """Spin-flip down and up, one channel: the ALDA0 kernel (density only: xc_sf) on ROKS
    and UKS, and the multicollinear LDA / GGA / MGGA kernels on ROKS."""
    from xtddft_amd.operator import DeviceOperator
    op_kind = "SF_DOWN" if isf == -1 else "SF_UP"
    case = _sf_case(xct, kind, isf, 1 if sf_kernel == "mc" else 0)
    mf = case[0]
    p = plan(mf, op_kind, nz, nc=5, no=2, sf_kernel=sf_kernel)
    assert_chunked(p, loops_meant(p, mf, nz, k_mode))
    if nz == 5 and op_kind == "SF_DOWN" and (xct == "LDA" or sf_kernel == "alda0"):
        assert p["xc"][0] == 234
    if nz == 5 and op_kind == "SF_DOWN" and xct == "GGA" and sf_kernel == "mc":
        assert p["xc"][0] == 163
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    kw = dict(sf_kernel="mc", mc_kernel=mf.fxc_sf_mc) if sf_kernel == "mc" else {}
    op = DeviceOperator(mf, op_kind, k_mode=k_mode, **kw)
    assert op.k_mode == k_mode
    _check(op, *_reference(case, nz))


@pytest.mark.parametrize("k_mode", ["direct", "stored"])
@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("sf_kernel", ["alda0", "mc"])
def test_xsf_chunked(hiplib, env, sf_kernel, nz, k_mode):
    """XSF with SA = 3 and the OO compression.  With the direct exchange the twelve Delta-A
    exchange products go through `sandwich`: at nz = 5 both of its branches run three aux
    chunks (30, 30, 18), the left one with beta = 0 on the first chunk and 1 afterwards.
    The J diagonals (over the whole factor) as in test_xsf."""
    from xtddft_amd.operator import DeviceOperator
    case = _xsf_case(1 if sf_kernel == "mc" else 0)
    mf, o, fg = case[0], case[1], case[2]
    p = plan(mf, "XSF", nz, nc=5, no=3, sf_kernel=sf_kernel)
    extra = ("sandwich_left", "sandwich_right") if (k_mode == "direct" and nz == 5) else ()
    assert_chunked(p, loops_meant(p, mf, nz, k_mode, extra))
    if nz == 5:
        assert p["sandwich_left_ov_cv"] == (30, 3, 18) and p["sandwich_right_cv_ov"] == (30, 3, 18)
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    kw = dict(sf_kernel="mc", mc_kernel=mf.fxc_sf_mc) if sf_kernel == "mc" else {}
    op = DeviceOperator(mf, "XSF", sa=3, fglobal=fg, foo=0.7, remove=True, k_mode=k_mode, **kw)
    assert o.re and op.k_mode == k_mode
    op.set_oo_basis(o.vects)
    _check(op, *_reference(case, nz))
    co, ov = op.xsf_j_diagonals()
    co_ref, ov_ref = o._response_j_diagonals()
    assert np.abs(co - co_ref).max() < 1e-13 and np.abs(ov - ov_ref).max() < 1e-13


def test_eri8_chunked(hiplib, env):
    """Stored ERIs: the Cholesky vectors of the packed ERIs (a device array) through the
    chunked df_to_mo, then the chunked grid, exchange and XC loops."""
    from xtddft_amd.operator import DeviceOperator
    case = _xtda_case("GGA", False, "RO")
    mf = case[0]
    p = plan(mf, "XTDA", 5, nc=5, no=2)
    assert_chunked(p, ["grid", "df", "exchange", "xc"])
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    op = DeviceOperator(as_eri8(mf), "XTDA", k_mode="direct")
    assert op.naux() == (mf.naux, mf.naux)
    _check(op, *_reference(case, 5), tol=ERI8_TOL)


def test_chunk_floors(hiplib, env):
    """The floors of the chunk rule, below any budget the other cases use: with
    XT_CHUNK_BYTES = 1 every quotient budget / bytes-per-row is 0 and the loops advance by
    one grid row (xt_set_grid), one aux row (df_to_mo, exchange_main) and 64 XC points."""
    from xtddft_amd.operator import DeviceOperator
    nz = 2
    mf = make_mf(nao=20, nc=5, no=2, naux=9, ngrid=150, xctype="GGA", hyb=0.2)
    vind, hdiag = oxtda.gen_tda_operation(mf)
    z = make_trial_vectors(nz, hdiag.size)
    p = plan(mf, "XTDA", nz, nc=5, no=2, budget=1)
    assert p == dict(grid=(1, 150, 1), xc=(64, 3, 22), df=(1, 9, 1), exchange0=(1, 9, 1))
    env(XT_CHUNK_BYTES=1)
    op = DeviceOperator(mf, "XTDA", k_mode="direct")
    r = rel(op.apply(z), vind(z))
    print(f"rel = {r:.3e}")
    assert r < RTOL


# ---- partitioned operator: the aux window together with p0 chunks -----------------------
@pytest.mark.parametrize("replicate", [False, True])
def test_partitioned_chunked(hiplib, env, replicate):
    """Three rank contexts (direct exchange), the factor aux-sliced or replicated with an
    aux window (bmo_of): every rank walks its 30 aux rows in chunks of 4 and its 600 grid
    points in chunks of 74; the parts sum to the oracle."""
    from xtddft_amd.operator import DeviceOperator
    nz = 5
    mf = make_mf(nao=30, nc=6, no=2, xctype="GGA", hyb=0.2, omega=0.3, alpha=0.6)
    vind, hdiag = oxtda.gen_tda_operation(mf)
    z = make_trial_vectors(nz, hdiag.size)
    assert mf.naux == 90 and mf.grids.ngrid == 1800
    p = plan(mf, "XTDA", nz, nc=6, no=2, naux=30, ngrid=600)       # the exchange / XC loops of one rank
    assert_chunked(p, ["grid", "exchange", "xc"])
    assert p["exchange0"] == (4, 8, 2) and p["xc"] == (74, 9, 8)
    if not replicate:      # df_to_mo of a 30-row slice (the whole factor is 10 chunks of 9)
        assert_chunked(p, ["df"])
    env(XT_CHUNK_BYTES=CHUNK_BYTES)
    parts = [DeviceOperator(mf, "XTDA", k_mode="direct", shard=(r, 3), replicate_df=replicate) for r in range(3)]
    assert all(q.replicate_df == replicate and q.k_mode == "direct" for q in parts)
    if replicate:
        assert [q.partition["aux"] for q in parts] == [(0, 30), (30, 60), (60, 90)]
    r = rel(sum(q.apply(z) for q in parts), vind(z))
    print(f"rel = {r:.3e}")
    assert r < RTOL


# ---- the fused XC kernels at g0 > 0 ------------------------------------------------------
@pytest.mark.parametrize("nz", [3, 7])
@pytest.mark.parametrize("nc,no,nao,knobs", [
    (99, 2, 130, dict()),                                   # dedicated rho-forward and M-backward
    (99, 2, 130, dict(XT_M_KERNEL=0, XT_W_KERNEL=0)),       # the engine's fused modes 1 and 2
    (33, 1, 60, dict(XT_W_KERNEL=3)),                       # the small-O rho-forward
    (140, 2, 163, dict()),                                  # the engine's mode 2 at O > 128
])
def test_fused_xc_kernels_chunked(hiplib, env, nc, no, nao, knobs, nz):
    """GGA X-TDA on 700 grid points in ten 64-point chunks and one of 60: every fused XC
    kernel reads PhiO / PhiV at a chunk offset g0 > 0 and its wv block with the zeroed
    slack rows after a ragged chunk."""
    from xtddft_amd.operator import DeviceOperator
    case = _xtda_case("GGA", False, "RO", nao=nao, nc=nc, no=no, ngrid=700)
    mf = case[0]
    p = plan(mf, "XTDA", nz, nc=nc, no=no)
    assert p["xc"] == (64, 11, 60)
    env(XT_CHUNK_BYTES=CHUNK_BYTES, **knobs)
    op = DeviceOperator(mf, "XTDA")
    _check(op, *_reference(case, nz))
