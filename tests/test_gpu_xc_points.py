"""GPU: every grid-point XC kernel variant of xt_kernels.hip at its dispatch boundaries,
against the oracle.

The launchers xc_uks_w, xc_sf and xc_uks_mgga pick a kernel and a template instance by xc
type, number of spin channels (NS) and the context's occupied row count O:

  family (operator, mean field, kernel)     O              kernel instance
  ----------------------------------------  -------------  ----------------------------------------
  X-TDA ROKS LDA  (xc_uks_w, ncomp 1)       64             k_xc_point<1,1,2>
                                            65, 128        k_xc_point<1,2,2>
                                            129, 256       k_xc_point<1,4,2>
                                            257            k_xc_uks_w<1,2>, one LDS image
  X-TDA ROKS GGA  (xc_uks_w, ncomp 4)       64             k_xc_point_b<4,1,2>
                                            65, 128        k_xc_point_b<4,2,2>
                                            129, 192       k_xc_point<4,4,2>, fourth register chunk empty
                                            193, 256       k_xc_point<4,4,2>, fourth register chunk in use
                                            257            k_xc_uks_w<4,2>, one LDS image
  U-TDA UKS LDA   (pO0 != pO1)              65             k_xc_point<1,2,2>
                                            129            k_xc_point<1,4,2>
                                            257            k_xc_uks_w<1,2>, two LDS images
  U-TDA UKS GGA   (pO0 != pO1)              64             k_xc_point_b<4,1,2>
                                            65, 128        k_xc_point_b<4,2,2>
                                            129, 193, 256  k_xc_point<4,4,2>
                                            257            k_xc_uks_w<4,2>, two LDS images
  X-TDA ROKS MGGA (xc_uks_mgga, ns 2)       64             k_xc_uks_mgga<2>, one 64-orbital stride
                                            65, 129, 257   k_xc_uks_mgga<2>, 2 / 3 / 5 strides, ragged
  U-TDA UKS MGGA                            64 ... 257     k_xc_uks_mgga<2>, two LDS images
  SF-down / SF-up ALDA0 (xc_sf)             128            k_xc_sf_pt<2>
                                            129, 192       k_xc_sf_pt<3>
                                            193, 256       k_xc_sf_pt<4>
                                            257            k_xc_sf
  XSF SA = 3 ALDA0 (xc_sf)                  129            k_xc_sf_pt<3>
                                            193            k_xc_sf_pt<4>
  SF-down multicollinear GGA                64             k_xc_point_b<4,1,1>
    (xc_uks_w, ns 1)                        65, 128        k_xc_point_b<4,2,1>
                                            129, 256       k_xc_point<4,4,1>
                                            257            k_xc_uks_w<4,1>
  SF-up multicollinear GGA                  65, 128        k_xc_point_b<4,2,1>
  SF-down multicollinear LDA (xc_sf)        129            k_xc_sf_pt<3>
                                            193            k_xc_sf_pt<4>
                                            257            k_xc_sf
  SF-down multicollinear MGGA               65, 257        k_xc_uks_mgga<1>
    (xc_uks_mgga, ns 1)

O is nc + no for X-TDA, U-TDA, SF-down and XSF and nc for SF-up (xt_create); each test
asserts it from nc, no.  A change of a dispatch boundary shows here which row moves.

Every case: ngrid = 203 (no multiple of 4: the last block of the one-wave-per-point
kernels has an idle wave), naux = 24, nv = 19, hyb = 0.2 (0.5 for the spin-flip kinds),
nz = 3 and 9 (below, and no multiple of, the 4- and 8-vector reduction batches);
1e-12 relative max-norm on sigma against the oracle, as in test_gpu_parity.py.
"""
import functools

import numpy as np
import pytest

from oracle import sf_tda as osf
from oracle import xsf_tda as oxsf
from oracle import xtda as oxtda
from xtddft_amd.synthetic import make_mf, make_trial_vectors

pytestmark = pytest.mark.gpu
RTOL = 1e-12
NGRID, NAUX, NV = 203, 24, 19
NZ = [3, 9]


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _mf(nc, no, xct, kind, hyb):
    return make_mf(nao=nc + no + NV, nc=nc, no=no, naux=NAUX, ngrid=NGRID, xctype=xct, kind=kind, hyb=hyb)


@functools.lru_cache(maxsize=None)
def _tda_case(xct, kind, O):
    nc, no = O - 2, 2
    mf = _mf(nc, no, xct, kind, 0.2)
    vind, hdiag = oxtda.gen_tda_operation(mf)
    return mf, nc, no, vind, hdiag.size


@functools.lru_cache(maxsize=None)
def _sf_case(xct, isf, method, O):
    nc, no = (O - 2, 2) if isf == -1 else (O, 2)
    mf = _mf(nc, no, xct, "RO", 0.5)
    vind, hdiag = osf.gen_tda_operation_sf(mf, isf, method=method)
    return mf, nc, no, vind, hdiag.size


@functools.lru_cache(maxsize=None)
def _xsf_case(O):
    nc, no = O - 3, 3
    mf = _mf(nc, no, "GGA", "RO", 0.5)
    o = oxsf.XSFOracle(mf, SA=3)
    fg = oxsf.default_fglobal(mf)
    # the preconditioner's J diagonals (setup, seconds at this O) are not part of A.x
    vind, hdiag = o.gen_tda_operation_sf(foo=0.7, fglobal=fg, with_hdiag=False)
    return mf, nc, no, o, fg, vind, hdiag.size


def _check(op, case, nz):
    vind, dim = case[-2], case[-1]
    z = make_trial_vectors(nz, dim)
    r = rel(op.apply(z), vind(z))
    print(f"rel = {r:.3e}")
    assert r < RTOL


def _context_rows(op):
    """The occupied row count O of the context, as xt_create sets it from the kind."""
    return op.nc if op.kind == "SF_UP" else op.nc + op.no


TDA = ([("LDA", "RO", O) for O in (64, 65, 128, 129, 256, 257)] +
       [("GGA", "RO", O) for O in (64, 65, 128, 129, 192, 193, 256, 257)] +
       [("LDA", "U", O) for O in (65, 129, 257)] +
       [("GGA", "U", O) for O in (64, 65, 128, 129, 193, 256, 257)] +
       [("MGGA", "RO", O) for O in (64, 65, 129, 257)] +
       [("MGGA", "U", O) for O in (64, 65, 129, 257)])


@pytest.mark.parametrize("nz", NZ)
@pytest.mark.parametrize("xct,kind,O", TDA)
def test_spin_conserving_point_kernels(hiplib, xct, kind, O, nz):
    """X-TDA on ROKS (one channel group, pO0 == pO1) and U-TDA on UKS (two groups, two
    occupied images): xc_uks_w for LDA / GGA, xc_uks_mgga for MGGA."""
    from xtddft_amd.operator import DeviceOperator
    case = _tda_case(xct, kind, O)
    mf, nc, no = case[:3]
    op = DeviceOperator(mf, "XTDA" if kind == "RO" else "UTDA")
    assert _context_rows(op) == nc + no == O and op.nv == NV
    _check(op, case, nz)


SF = ([("GGA", isf, 0, O) for isf in (-1, 1) for O in (128, 129, 192, 193, 256, 257)] +     # ALDA0
      [("GGA", -1, 1, O) for O in (64, 65, 128, 129, 256, 257)] +
      [("GGA", 1, 1, O) for O in (65, 128)] +
      [("LDA", -1, 1, O) for O in (129, 193, 257)] +
      [("MGGA", -1, 1, O) for O in (65, 257)])


@pytest.mark.parametrize("nz", NZ)
@pytest.mark.parametrize("xct,isf,method,O", SF)
def test_spin_flip_point_kernels(hiplib, xct, isf, method, O, nz):
    """One spin-flip channel: ALDA0 (method 0, GGA mean field, density only) and the
    multicollinear LDA kernel through xc_sf; the multicollinear GGA / MGGA kernels through
    the one-channel instances of xc_uks_w / xc_uks_mgga."""
    from xtddft_amd.operator import DeviceOperator
    case = _sf_case(xct, isf, method, O)
    mf, nc, no = case[:3]
    kw = dict(sf_kernel="mc", mc_kernel=mf.fxc_sf_mc) if method == 1 else {}
    op = DeviceOperator(mf, "SF_DOWN" if isf == -1 else "SF_UP", **kw)
    assert _context_rows(op) == (nc + no if isf == -1 else nc) == O and op.nv == NV
    _check(op, case, nz)


@pytest.mark.parametrize("nz", NZ)
@pytest.mark.parametrize("O", [129, 193])
def test_xsf_point_kernels(hiplib, O, nz):
    """XSF with SA = 3 and the OO compression, ALDA0: xc_sf at O = nc + no."""
    from xtddft_amd.operator import DeviceOperator
    case = _xsf_case(O)
    mf, nc, no, o, fg = case[:5]
    op = DeviceOperator(mf, "XSF", sa=3, fglobal=fg, foo=0.7, remove=True)
    assert _context_rows(op) == nc + no == O and op.nv == NV
    op.set_oo_basis(o.vects)
    _check(op, case, nz)
