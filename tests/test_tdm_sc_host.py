"""CPU: the spin-conserving transition-moment restatement (tests/xtda_tdm_ref.py) and the host
side of ``xt_tdm_sc`` (declaration, export, descriptor layout, argument validation before any
HIP call, the ``XTDA`` methods)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import xtda_tdm_ref as ref
from xtddft_amd.utils import order_pyscf2my

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xtddft_amd.h")

SHAPES = [(3, 2, 5), (5, 3, 7), (2, 2, 1)]


def problem(nc, no, nv, nstates, ncomp, seed=0):
    """Random states in PySCF order [za | zb], a random symmetric operator over [c|o|v]."""
    rng = np.random.default_rng(seed)
    nmo = nc + no + nv
    vecs = rng.standard_normal((nstates, (nc + no) * nv + nc * (no + nv)))
    d = rng.standard_normal((ncomp, nmo, nmo))
    return vecs, d + d.transpose(0, 2, 1)


def so_form(vecs, d, nc, no, nv, ground=True):
    """``tdm_so`` on the un-rotated (za, zb) of a ROKS reference: alpha [c o | v], beta [c | o v]."""
    return ref.tdm_so(vecs, d, d, nc + no, nv, nc, no + nv, ground)


# ---- yardstick: the restatement itself -------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(6, 0, 9)])
def test_restatement_is_symmetric_and_origin_independent(shape):
    nc, no, nv = shape
    vecs, d = problem(nc, no, nv, 4, 3)
    shift = np.array([0.7, -1.3, 2.1])[:, None, None] * np.eye(nc + no + nv)
    for t, t2 in ((ref.tdm_xtda(vecs, d, nc, no, nv, no / 2), ref.tdm_xtda(vecs, d + shift, nc, no, nv, no / 2)),
                  (so_form(vecs, d, nc, no, nv), so_form(vecs, d + shift, nc, no, nv))):
        scale = np.abs(t).max()
        assert t.shape == (3, 5, 5)
        assert np.abs(t - t.transpose(0, 2, 1)).max() < 1e-13 * scale
        # c 1 (the overlap in the MO basis) adds nothing, ground row and diagonal included
        assert np.abs(t2 - t).max() < 1e-12 * scale
        assert np.all(t[:, 0, 0] == 0.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_pin_minus_g_reduces_to_the_spin_orbital_form(shape):
    """With g forced to 1/sqrt(2) the spin-adapted restatement (-g in so2st's phase) is the
    spin-orbital formula on the un-rotated amplitudes; with +g (tdm.py's sign, written for a
    CV(1) of the opposite phase) it is not."""
    nc, no, nv = shape
    vecs, d = problem(nc, no, nv, 5, 3, seed=1)
    so = so_form(vecs, d, nc, no, nv)
    t = ref.tdm_xtda(vecs, d, nc, no, nv, no / 2, g=1 / np.sqrt(2))
    assert np.abs(t - so).max() < 1e-13 * np.abs(so).max()
    plus = ref.tdm_xtda(vecs, d, nc, no, nv, no / 2, g=-1 / np.sqrt(2))
    assert np.abs(plus - so).max() > 1e-3 * np.abs(so).max()
    # and the real g changes something
    assert np.abs(ref.tdm_xtda(vecs, d, nc, no, nv, no / 2) - so).max() > 1e-3 * np.abs(so).max()


def test_closed_shell_restatement_equals_the_spin_orbital_form():
    nc, no, nv = 6, 0, 9
    vecs, d = problem(nc, no, nv, 5, 3, seed=2)
    so = so_form(vecs, d, nc, no, nv)
    assert np.abs(ref.tdm_xtda(vecs, d, nc, no, nv, 0.0) - so).max() < 1e-13 * np.abs(so).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_ground_row_equals_the_contraction_of_xtda_transition(shape):
    """XTDA._transition's einsum lines on random vectors in "my order" against TDM_GSS."""
    nc, no, nv = shape
    rng = np.random.default_rng(3)
    nmo = nc + no + nv
    vecs, _ = problem(nc, no, nv, 4, 3, seed=3)
    c = rng.standard_normal((nmo, nmo))
    op_ao = rng.standard_normal((3, nmo, nmo))
    op_ao = op_ao + op_ao.transpose(0, 2, 1)
    order = order_pyscf2my(nc, no, nv)
    v = vecs.T[order, :]                                   # what XTDA.Davidson stores
    coa, cva, cob, cvb = c[:, :nc + no], c[:, nc + no:], c[:, :nc], c[:, nc:]
    a = np.einsum('xpq,pi,qj->xij', op_ao, coa, cva).reshape(3, -1)
    b = np.einsum('xpq,pi,qj->xij', op_ao, cob, cvb).reshape(3, -1)
    na = (nc + no) * nv
    b = b[:, order[na:] - na]
    vt = v.T
    tdip = np.einsum('xi,yi->yx', a, vt[:, :na]) + np.einsum('xi,yi->yx', b, vt[:, na:])
    d = np.einsum('xpq,pi,qj->xij', op_ao, c, c)
    t0 = ref.tdm_gss(vecs, d, nc, no, nv)
    assert np.abs(tdip.T - t0).max() < 1e-13 * np.abs(t0).max()
    assert np.array_equal(ref.tdm_xtda(vecs, d, nc, no, nv, no / 2)[:, 0, 1:], t0)


# ---- feature: the entry's host side ------------------------------------------
def test_header_declares_and_library_exports_xt_tdm_sc(hiplib):
    txt = open(HEADER).read()
    assert re.search(r"^\s*int\s+xt_tdm_sc\s*\(", txt, re.M)
    assert "XT_ABI_VERSION 8" in txt
    assert hasattr(hiplib, "xt_tdm_sc")
    from xtddft_amd import _capi, build
    assert "xt_tdm_sc" in _capi.EXPORTS and "xt_tdm_sc.hip" in build.SOURCES


def test_tdm_sc_desc_layout_matches_c_header(tmp_path):
    from xtddft_amd._capi import XtTdmScDesc
    fields = [f for f, _ in XtTdmScDesc._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xtddft_amd.h"\nint main(){'
                   'printf("%zu", sizeof(xt_tdm_sc_desc));' +
                   "".join(f'printf(" %zu", offsetof(xt_tdm_sc_desc, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(XtTdmScDesc)
    assert out[1:] == [getattr(XtTdmScDesc, f).offset for f in fields]


def test_xt_tdm_sc_rejects_bad_arguments_without_gpu(hiplib):
    """Every validation case returns XT_ERR_ARG (-1) with a message before any HIP call."""
    from xtddft_amd import _capi
    nc, no, nv, n = 3, 2, 5, 4
    nao = nc + no + nv
    op = np.zeros((3, nao, nao))
    cs = [np.zeros((nao, k)) for k in (nc + no, nv, nc, no + nv)]
    vecs = np.zeros((n, (nc + no) * nv + nc * (no + nv)))
    out = np.zeros((3, n + 1, n + 1))

    def call(null=None, desc=True, ptr_kind=_capi.XT_PTR_HOST, **kw):
        f = dict(nao=nao, nocc_a=nc + no, nvir_a=nv, nocc_b=nc, nvir_b=no + nv, ncomp=3, nstates=n,
                 spin_adapted=1, no=no, si=no / 2, with_ground=1)
        f.update(kw)
        d = _capi.XtTdmScDesc(**f)
        ptrs = dict(op=op, coa=cs[0], cva=cs[1], cob=cs[2], cvb=cs[3], vecs=vecs, out=out)
        args = [None if k == null else a.ctypes.data for k, a in ptrs.items()]
        rc = hiplib.xt_tdm_sc(ctypes.byref(d) if desc else None, *args, ptr_kind, None)
        return rc, hiplib.xt_last_error()

    rc, msg = call(desc=False)
    assert rc == -1 and b"descriptor" in msg
    for k in ("op", "coa", "cva", "cob", "cvb", "vecs", "out"):
        rc, msg = call(null=k)
        assert rc == -1 and b"null" in msg, k
    for k in ("nao", "ncomp", "nstates"):
        rc, msg = call(**{k: 0})
        assert rc == -1 and k.encode() in msg, k
    rc, msg = call(nvir_a=-1)
    assert rc == -1 and b"counts" in msg
    rc, msg = call(nocc_a=0, nvir_a=0, nocc_b=0, nvir_b=0, spin_adapted=0)
    assert rc == -1 and b"counts" in msg
    rc, msg = call(nocc_a=nc + no + 1)                    # nocc_a - nocc_b != no
    assert rc == -1 and b"ROKS" in msg
    rc, msg = call(nvir_b=no + nv - 1)                    # nvir_b - nvir_a != no
    assert rc == -1 and b"ROKS" in msg
    rc, msg = call(no=no + 1)
    assert rc == -1 and b"ROKS" in msg
    for si in (0.0, -1.0):
        rc, msg = call(si=si)
        assert rc == -1 and b"S > 0" in msg
    with pytest.raises(ValueError, match="S > 0"):
        _capi.check(rc, "xt_tdm_sc")
    rc, msg = call(ptr_kind=2)
    assert rc == -1 and b"ptr_kind" in msg
    # the same counts are fine without spin adaptation -- then only ptr_kind is left to refuse
    rc, msg = call(spin_adapted=0, nocc_a=nc + no + 1, si=0.0, ptr_kind=7)
    assert rc == -1 and b"ptr_kind" in msg


def test_xtda_has_the_moment_methods():
    from xtddft_amd.xtda import XTDA
    for name in ("transition_dipoles", "osc_matrix", "state_dipoles", "calculate_TDM"):
        assert callable(getattr(XTDA, name, None)), name


@pytest.mark.parametrize("kind", ["R", "U"])
def test_default_dipole_needs_a_mole_with_integrals(kind):
    """Without a Mole that has integrals the default-operator path raises ValueError, as
    XTDA.osc_str does."""
    from xtddft_amd.synthetic import make_mf
    from xtddft_amd.xtda import XTDA
    mf = make_mf(nao=12, nc=3, no=2) if kind == "R" else make_mf(nao=12, nc=3, no=2, kind="U")
    x = XTDA(None, mf, nstates=3)
    for call in (x.transition_dipoles, x.osc_matrix, x.state_dipoles, x.calculate_TDM):
        with pytest.raises(ValueError, match="dipole"):
            call()


def test_tables_follow_the_reference_lines():
    from xtddft_amd import tdm
    rng = np.random.default_rng(5)
    n = 4
    t, e = rng.standard_normal((3, n + 1, n + 1)), np.sort(rng.random(n))
    lines = tdm.tdm_tables_sc(e, t)
    assert len(lines) == (1 + n) + 1 + 2 + n * n
    assert lines[0] == "Ground state to Excited state transition dipole moments(a.u.)"
    i = 2
    f = 2 / 3 * e[i] * (t[:, i + 1, 0] ** 2).sum()
    assert lines[1 + i] == (f' {i + 1:2d}     |GS⟩    {t[0, i + 1, 0]:>8.4f} {t[1, i + 1, 0]:>8.4f} '
                            f'{t[2, i + 1, 0]:>8.4f}  {f:>8.4f} ')
    assert lines[n + 1] == ""
    assert lines[n + 2] == "Excited state to Excited state transition dipole moments(a.u.)"
    assert lines[n + 3] == "StateL StateR      X        Y        Z      f(L<-R)"
    i, j = 1, 3
    tt = t[:, i + 1, j + 1]
    f = 2 / 3 * (e[i] - e[j]) * (tt ** 2).sum()
    assert lines[n + 4 + i * n + j] == (f' {i + 1:2d}     {j + 1:2d}    {tt[0]:>8.4f} {tt[1]:>8.4f} {tt[2]:>8.4f}  '
                                        f'{f:>8.4f} ')
    o = tdm.osc_matrix(np.concatenate([[0.0], e]), t)
    assert np.abs(o - ref.osc(np.concatenate([[0.0], e]), t)).max() < 1e-15
