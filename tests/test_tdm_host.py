"""CPU: the transition-moment restatement (tests/tdm_ref.py) and the host side of ``xt_tdm``
(declaration, export, argument validation before any HIP call, Python methods)."""
import ctypes
import os
import re

import numpy as np
import pytest

import tdm_ref
from oracle.xsf_tda import get_vect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xtddft_amd.h")


def problem(nc, no, nv, nstates, ncomp, compressed, seed=0):
    """Random states (block rows), a random symmetric operator in the MO basis."""
    rng = np.random.default_rng(seed)
    nmo = nc + no + nv
    dim = (nc + no) * (no + nv) - (1 if compressed else 0)
    vecs = rng.standard_normal((nstates, dim))
    d = rng.standard_normal((ncomp, nmo, nmo))
    d = d + d.transpose(0, 2, 1)
    vects = get_vect(no) if compressed else None
    return vecs, d, vects


# ---- yardstick: the restatement itself -------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 5), (5, 3, 7), (2, 2, 1)])
@pytest.mark.parametrize("sa", [0, 3])
@pytest.mark.parametrize("compressed", [False, True])
def test_restatement_is_symmetric_and_origin_independent(shape, sa, compressed):
    nc, no, nv = shape
    vecs, d, vects = problem(nc, no, nv, 4, 3, compressed)
    t = tdm_ref.tdm_roks(vecs, d, nc, no, nv, sa, no / 2, vects)
    scale = np.abs(t).max()
    assert np.abs(t - t.transpose(0, 2, 1)).max() < 1e-13 * scale
    # an operator proportional to the overlap (the identity in the MO basis) adds nothing:
    # the moments do not depend on the dipole origin, diagonal ones included
    shift = np.array([0.7, -1.3, 2.1])[:, None, None] * np.eye(nc + no + nv)
    t2 = tdm_ref.tdm_roks(vecs, d + shift, nc, no, nv, sa, no / 2, vects)
    assert np.abs(t2 - t).max() < 1e-12 * scale


@pytest.mark.parametrize("shape", [(3, 2, 5), (5, 3, 7), (2, 2, 1), (6, 0, 9)])
def test_restatement_roks_at_sa0_equals_uks_form(shape):
    nc, no, nv = shape
    vecs, d, _ = problem(nc, no, nv, 5, 3, False, seed=1)
    t = tdm_ref.tdm_roks(vecs, d, nc, no, nv, 0, no / 2)
    u = tdm_ref.tdm_uks(vecs, d[:, :nc + no, :nc + no], d[:, nc:, nc:], nc, no, nv)
    assert np.abs(t - u).max() < 1e-13 * np.abs(t).max()


def test_restatement_block_rows_roundtrip():
    nc, no, nv = 3, 2, 5
    c = np.random.default_rng(2).standard_normal((4, nc + no, no + nv))
    cv, co, ov, oo = tdm_ref.split_blocks(tdm_ref.blocks_to_rows(c, nc, no, nv), nc, no, nv)
    assert np.array_equal(cv, c[:, :nc, no:]) and np.array_equal(co, c[:, :nc, :no])
    assert np.array_equal(ov, c[:, nc:, no:]) and np.array_equal(oo, c[:, nc:, :no])


# ---- feature: the entry's host side ------------------------------------------
def test_header_declares_and_library_exports_xt_tdm(hiplib):
    txt = open(HEADER).read()
    assert re.search(r"^\s*int\s+xt_tdm\s*\(", txt, re.M)
    assert "XT_ABI_VERSION 8" in txt
    assert hasattr(hiplib, "xt_tdm")
    from xtddft_amd import _capi, build
    assert "xt_tdm" in _capi.EXPORTS and "xt_tdm.hip" in build.SOURCES


def test_tdm_desc_layout_matches_c_header(tmp_path):
    import subprocess
    from xtddft_amd._capi import XtTdmDesc
    fields = [f for f, _ in XtTdmDesc._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xtddft_amd.h"\nint main(){'
                   'printf("%zu", sizeof(xt_tdm_desc));' +
                   "".join(f'printf(" %zu", offsetof(xt_tdm_desc, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(XtTdmDesc)
    assert out[1:] == [getattr(XtTdmDesc, f).offset for f in fields]


def test_xt_tdm_rejects_bad_arguments_without_gpu(hiplib):
    """Every validation case returns XT_ERR_ARG (-1) before any HIP call."""
    from xtddft_amd import _capi
    nc, no, nv, n = 3, 2, 5, 4
    nao = nc + no + nv
    op = np.zeros((3, nao, nao))
    co, cv = np.zeros((nao, nc + no)), np.zeros((nao, no + nv))
    vecs = np.zeros((n, (nc + no) * (no + nv)))
    vects = np.zeros((no * no, no * no - 1))
    out = np.zeros((3, n, n))

    def call(vects_arg=None, **kw):
        f = dict(nao=nao, nc=nc, no=no, nv=nv, ncomp=3, nstates=n, sa=0, si=no / 2, layout=1, oo_compressed=0)
        f.update(kw)
        d = _capi.XtTdmDesc(**f)
        rc = hiplib.xt_tdm(ctypes.byref(d), op.ctypes.data, co.ctypes.data, cv.ctypes.data, vecs.ctypes.data,
                           None if vects_arg is None else vects_arg.ctypes.data, out.ctypes.data,
                           _capi.XT_PTR_HOST, None)
        return rc, hiplib.xt_last_error()

    assert call(ncomp=0)[0] == -1
    assert call(nstates=0)[0] == -1
    rc, msg = call(layout=2)
    assert rc == -1 and b"layout" in msg
    assert call(oo_compressed=1)[0] == -1                                   # compressed, no vects
    assert call(vects_arg=vects, oo_compressed=1, no=0, nv=nv + no)[0] == -1     # compressed, no open shell
    rc, msg = call(sa=3, si=0.5, no=1, nv=nv + 1)                            # 2S-1 = 0
    assert rc == -1 and b"2S-1" in msg
    with pytest.raises(ValueError):
        _capi.check(rc, "xt_tdm")
    assert call(sa=3, si=0.0, no=0, nv=nv + no)[0] == -1


def test_spin_flip_classes_have_the_moment_methods():
    from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up
    from xtddft_amd.xsf_tda import XSF_TDA
    for cls in (XSF_TDA, SF_TDA_down, SF_TDA_up):
        assert callable(getattr(cls, "transition_dipoles", None)), cls
        assert callable(getattr(cls, "osc_str", None)), cls
    assert callable(getattr(XSF_TDA, "calculate_TDM", None))


def test_default_dipole_needs_a_mole_with_integrals():
    """Without a Mole that has integrals the methods raise ValueError, as XTDA.osc_str does."""
    from xtddft_amd.sf_tda import SF_TDA_up
    from xtddft_amd.synthetic import make_mf
    from xtddft_amd.xsf_tda import XSF_TDA
    mf = make_mf(nao=12, nc=3, no=2)
    for obj in (XSF_TDA(mf), SF_TDA_up(mf)):
        with pytest.raises(ValueError, match="dipole"):
            obj.transition_dipoles()
        with pytest.raises(ValueError, match="dipole"):
            obj.osc_str()


def test_osc_matrix_and_table_follow_the_reference_lines():
    from xtddft_amd import tdm
    rng = np.random.default_rng(5)
    t, e = rng.standard_normal((3, 4, 4)), np.sort(rng.standard_normal(4))
    o = tdm.osc_matrix(e, t)
    assert np.array_equal(o, tdm_ref.osc(e, t)) or np.abs(o - tdm_ref.osc(e, t)).max() < 1e-15
    lines = tdm.tdm_table(t, o)
    assert lines[1] == "State State    X     Y     Z     OSC." and len(lines) == 2 + 16
    i, j = 1, 2
    assert lines[2 + i * 4 + j] == (f'{i + 1:2d} {j + 1:2d} {t[0, i, j]:>8.4f} {t[1, i, j]:>8.4f} '
                                    f'{t[2, i, j]:>8.4f}  {o[i, j]:>8.4f} ')
