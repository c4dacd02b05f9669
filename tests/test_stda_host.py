"""sX-TDA / sU-TDA on the host: the C ABI's struct layouts and argument checks (no GPU), and the
NumPy restatement tests/stda_ref.py pinned to the reference's own printed sU-TDA run
(example/sTDA.ipynb: CH2O+, UKS B3LYP/cc-pVDZ, vacuum; tests/golden/stda_reference_outputs.json).
The GPU tests compare the device against that restatement."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import stda_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "xtddft_amd.h")
PRINT_TOL = 6e-5          # the 4-decimal print (tests/test_qc.py TD_PRINT_TOL_EV)
NAMES = ("xt_stda_charges", "xt_stda_half", "xt_stda_diag", "xt_stda_select", "xt_stda_matrix")


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


# --------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("cname,pyname", [("xt_stda_desc", "XtStdaDesc"), ("xt_stda_ops", "XtStdaOps")])
def test_stda_struct_layouts_match_c_header(tmp_path, cname, pyname):
    from xtddft_amd import _capi
    cls = getattr(_capi, pyname)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xtddft_amd.h"\nint main(){'
                   f'printf("%zu", sizeof({cname}));' +
                   "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, f).offset for f in fields]


def test_stda_entries_are_declared_everywhere():
    from xtddft_amd import _capi, build
    header = open(HEADER).read()
    for n in NAMES:
        assert n in _capi.EXPORTS and f"int {n}(" in header
    assert "os_sTDA.py" in header
    assert "xt_stda.hip" in build.SOURCES
    assert _capi.ABI_VERSION == 8


def test_stda_entries_reject_bad_arguments_without_gpu(hiplib):
    """Every entry validates before the first HIP call: XT_ERR_ARG (-1) with its own message on a
    machine without a device -- not XT_ERR_HIP (-3) from a failed HIP call."""
    from xtddft_amd import _capi
    L = hiplib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ip = ctypes.POINTER(ctypes.c_int)

    def ints(v):
        a = np.ascontiguousarray(v, dtype=np.int32)
        return a, a.ctypes.data_as(ip)

    def desc(**kw):
        d = dict(natm=2, nocc_a=3, nvir_a=2, nocc_b=2, nvir_b=3, nc=2, no=1, nv=2, spin_adapted=1, si=0.5,
                 correct=0, delta_max=0.0, sigma_k=0.0)
        d.update(kw)
        return _capi.XtStdaDesc(**d)

    def ops(**kw):
        o = _capi.XtStdaOps(**{f"{n}_{s}": p for s in "ab" for n in _capi.STDA_OPS})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    good = [[0, 0, 0], [0, 2, 1], [1, 1, 0], [1, 0, 2]]
    _, off = ints([0, 1, 4])

    def charges(d=None, spin=0, nao=4, off=off, c=p, qoo=p, qov=p, qvv=p):
        return L.xt_stda_charges(ctypes.byref(d or desc()), spin, nao, off, c, qoo, qov, qvv, None)

    def half(d=None, spin=0, gk=p, gj=p, qov=p, qvv=p, kov=p, jvv=p):
        return L.xt_stda_half(ctypes.byref(d or desc()), spin, gk, gj, qov, qvv, kov, jvv, None)

    def diag(d=None, o=None, csf=good, n=None, e=p):
        keep, c = ints(csf)
        return L.xt_stda_diag(ctypes.byref(d or desc()), ctypes.byref(o or ops()), len(csf) if n is None else n,
                              c if csf is not None and len(csf) else None, e, p, None)

    def select(d=None, o=None, csf=good, n=None, e=p, w=p):
        keep, c = ints(csf)
        m = len(csf) if n is None else n
        cp = c if len(csf) else None
        return L.xt_stda_select(ctypes.byref(d or desc()), ctypes.byref(o or ops()), m, cp, e, m, cp, e, w, None)

    def matrix(d=None, o=None, csf=good, n=None, e=p):
        keep, c = ints(csf)
        return L.xt_stda_matrix(ctypes.byref(d or desc()), ctypes.byref(o or ops()), len(csf) if n is None else n,
                                c if len(csf) else None, e, None)

    def msg():
        return L.xt_last_error().decode()

    # descriptor: negative sizes, flags, ROKS consistency, S
    for name, f in (("xt_stda_charges", charges), ("xt_stda_half", half), ("xt_stda_diag", diag),
                    ("xt_stda_select", select), ("xt_stda_matrix", matrix)):
        for bad in (dict(natm=-1), dict(nocc_a=-1), dict(nvir_b=-2), dict(nv=-1), dict(spin_adapted=2),
                    dict(correct=-1), dict(nocc_a=2), dict(si=0.0), dict(si=-0.5), dict(correct=1, sigma_k=0.0)):
            assert f(d=desc(**bad)) == -1, (name, bad)
            assert msg().startswith(name + ":"), msg()
    assert charges(d=desc(natm=0)) == 0 and half(d=desc(natm=0)) == 0          # no work: nothing touched
    assert charges(d=desc(natm=0), off=None, c=None, qoo=None, qov=None, qvv=None) == 0
    assert half(d=desc(natm=0), gk=None, gj=None, qov=None, qvv=None, kov=None, jvv=None) == 0
    # charges: spin, nao, offsets, null pointers
    assert charges(spin=2) == -1 and charges(nao=-1) == -1 and charges(off=None) == -1
    assert charges(off=ints([0, 3, 2])[1]) == -1 and "decrease" in msg()
    assert charges(off=ints([0, 1, 5])[1]) == -1 and charges(off=ints([-1, 1, 4])[1]) == -1
    for name in ("c", "qoo", "qov", "qvv"):
        assert charges(**{name: None}) == -1 and msg().startswith("xt_stda_charges:")
    # half
    assert half(spin=-1) == -1
    for name in ("gk", "gj", "qov", "qvv", "kov", "jvv"):
        assert half(**{name: None}) == -1 and msg().startswith("xt_stda_half:")
    # the three list consumers: length, indices outside their block, null pointers
    for name, f in (("xt_stda_diag", diag), ("xt_stda_select", select), ("xt_stda_matrix", matrix)):
        assert f(n=-1) == -1 and msg().startswith(name + ":")
        for entry in ([2, 0, 0], [-1, 0, 0], [0, 3, 0], [0, 0, 2], [1, 2, 0], [1, 0, 3], [0, -1, 0], [1, 0, -1]):
            assert f(csf=good + [entry]) == -1, (name, entry)
            assert msg().startswith(name + ":") and "entry 4" in msg(), msg()
        assert f(e=None) == -1
        for field in ("q_ov_a", "k_ov_b", "q_oo_a", "j_vv_b"):
            assert f(o=ops(**{field: None})) == -1 and msg().startswith(name + ":")
        assert f(csf=[]) == 0                                                  # empty list: nothing touched
        assert f(csf=[], e=None, o=ops(q_ov_a=None)) == 0
    for f in (diag, matrix):     # the full generator also needs the Fock blocks
        for field in ("f_oo_a", "f_vv_b", "h_oo_a", "h_vv_b"):
            assert f(o=ops(**{field: None})) == -1
        # spin-orbital: S is not used, so si = 0 is no error (empty work: nothing is launched)
        assert f(d=desc(spin_adapted=0, si=0.0), csf=[]) == 0
    assert select(w=None) == -1
    assert L.xt_abi_version() == 8


# --------------------------------------------------------------------------- the restatement vs the notebook
@pytest.fixture(scope="module")
def ch2o():
    from molecules import tda_meanfield
    mf = tda_meanfield("CH2O_UKS")
    mol = mf.extra["qc_mol"]
    eta = golden("stda_eta.json")["eta_eV"]
    xyz = mol.atom_coords()
    dist = np.linalg.norm(xyz[:, None] - xyz[None], axis=2)
    off = np.searchsorted(mol.ao_atom(), np.arange(mol.natm + 1))
    pr, orbs, lo = ref.problem_from_mf(mf, False, 10.0, True, False, 'os', [eta[e] for e in mol.elements], off, dist)
    e, v, a, ps, counts, w = ref.solve(pr, 10.0, union=True, nstates=12)
    return dict(mf=mf, mol=mol, pr=pr, orbs=orbs, lo=lo, e=e, v=v, a=a, ps=ps, counts=counts, w=w)


def test_restatement_reproduces_the_notebook_counts(ch2o):
    g = golden("stda_reference_outputs.json")["sutda_ch2o"]
    pr, c = ch2o["pr"], ch2o["counts"]
    info = ch2o["mf"].shape_info()
    assert (info["nc"], info["no"], info["nv"]) == (g["full_space"]["nc"], g["full_space"]["no"], g["full_space"]["nv"])
    assert (info["nc"] + info["no"]) * info["nv"] + info["nc"] * (info["no"] + info["nv"]) == g["full_space"]["dim"]
    assert ch2o["mf"].hyb == g["hyb"]
    assert (pr["nc"], pr["no"], pr["nv"]) == (5, 1, 9)
    assert (c["p_cva_before_union"], c["p_cvb_before_union"]) == (g["pcsf_before_union"]["cv_a"], g["pcsf_before_union"]["cv_b"])
    assert (c["s_cva_before_union"], c["s_cvb_before_union"]) == (g["scsf_before_union"]["cv_a"], g["scsf_before_union"]["cv_b"])
    assert c["pcsf"] == g["pcsf"]
    assert [t - p for t, p in zip(c["pscsf"], c["pcsf"])] == g["scsf"]
    assert c["pscsf"] == [17, 3, 4, 17]
    assert ch2o["a"].shape == (g["dim"], g["dim"]) and sum(c["pscsf"]) == g["dim"]
    assert c["ncsf"] == g["ncsf"]


def test_restatement_reproduces_the_notebook_roots_and_properties(ch2o):
    g = golden("stda_reference_outputs.json")["sutda_ch2o"]
    pr = ch2o["pr"]
    e_ev = ch2o["e"] * ref.HA2EV
    err = np.abs(e_ev - np.array(g["energy_eV"])).max()
    print("roots vs print (eV)", err)
    assert err < PRINT_TOL
    f = ref.osc_str(ch2o["e"], ch2o["v"], ch2o["ps"], ch2o["mol"].intor_symmetric("int1e_r", comp=3), *ch2o["orbs"],
                    pr["nc"], pr["no"])
    ds = ref.delta_s2_so(ch2o["v"], ch2o["ps"], ch2o["mf"].get_ovlp(), *ch2o["orbs"], pr["nc"], pr["no"], pr["nv"])
    print("f vs print", np.abs(f - np.array(g["osc_str"])).max(), "dS2 vs print", np.abs(ds - np.array(g["deltaS2"])).max())
    assert np.abs(f - np.array(g["osc_str"])).max() < PRINT_TOL
    assert np.abs(ds - np.array(g["deltaS2"])).max() < PRINT_TOL


def test_no_selection_weight_sits_at_the_threshold(ch2o):
    """A condition on the input: round-off cannot flip the selected set."""
    w = ch2o["w"]
    assert w.size == 96
    ratio = np.exp(np.abs(np.log(w / ref.TP)).min())
    print("closest weight to tp: factor", ratio)
    assert ratio > 1.01


def test_restatement_is_consistent_with_itself(ch2o):
    """diag is the diagonal of matrix; the A of the selected list is the cut of the A of the
    whole active space; both triangles agree."""
    pr, ps = ch2o["pr"], ch2o["ps"]
    nc, no, nv = pr["nc"], pr["no"], pr["nv"]
    csf = np.concatenate([ref.to_triples(k, *ps[k], nc, no) for k in range(4)])
    a = ref.matrix(pr, csf)
    assert np.abs(a - a.T).max() < 1e-13
    e, k = ref.diag(pr, csf)
    assert np.abs(e - np.diag(a)).max() < 1e-14
    every = np.concatenate([ref.to_triples(c, *lst, nc, no) for c, lst in enumerate(ref.class_lists(nc, no, nv))])
    full = ref.matrix(pr, every)
    pos = {tuple(t): n for n, t in enumerate(every)}
    idx = [pos[tuple(t)] for t in csf]
    assert np.abs(full[np.ix_(idx, idx)] - a).max() < 1e-14


def test_host_class_validates_its_arguments():
    from xtddft_amd import OSsTDA
    from xtddft_amd.synthetic import make_mf
    ro, u = make_mf(nao=12, nc=3, no=1, kind="RO"), make_mf(nao=12, nc=3, no=1, kind="U")
    atoms = dict(elements=["C", "H", "Xx"], atom_coords=np.eye(3), ao_atom=[0] * 5 + [1] * 6 + [2])
    eta = golden("stda_eta.json")["eta_eV"]
    with pytest.raises(ValueError, match="Xx"):
        OSsTDA(None, ro, eta=eta, **atoms)
    with pytest.raises(ValueError, match="required"):
        OSsTDA(None, ro, **atoms)
    eta = dict(eta, Xx=5.0)
    with pytest.raises(ValueError, match="ROKS"):
        OSsTDA(None, u, spinadapt=True, eta=eta, **atoms)
    with pytest.raises(ValueError, match="UKS"):
        OSsTDA(None, ro, spinadapt=False, eta=eta, **atoms)
    with pytest.raises(ValueError, match="ao_atom"):
        OSsTDA(None, ro, eta=eta, **dict(atoms, ao_atom=[0, 1] * 6))
    with pytest.raises(ValueError, match="atoms"):
        OSsTDA(None, ro, eta=eta)
    x = OSsTDA(None, ro, eta=eta, **atoms)
    assert x.tp == 1e-4 and x.Emax == 10.0 and x.natm == 3 and list(x.ao_off) == [0, 5, 11, 12]
    gj, gk = x.gamma(0.2)
    d = np.sqrt(2.0) * (1 - np.eye(3))
    rj, rk = ref.gamma(d, [eta[e] for e in atoms["elements"]], 0.2, "os")
    assert np.abs(gj - rj).max() < 1e-15 and np.abs(gk - rk).max() < 1e-15
