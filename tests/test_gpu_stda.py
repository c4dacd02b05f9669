"""GPU: the sX-TDA / sU-TDA entry points (``xt_stda_charges / _half / _diag / _select / _matrix``)
and the ``OSsTDA`` driver against the term-by-term NumPy restatement tests/stda_ref.py of
xtddft/sTDA/os_sTDA.py, and the driver against the reference's printed sU-TDA run
(tests/golden/stda_reference_outputs.json).

The tolerance is the project's RTOL for device-vs-oracle FP64 contractions
(tests/test_gpu_tdm_sc.py): max|dev - ref| / max|ref| < 1e-12."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import stda_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
PRINT_TOL = 6e-5

NATM = [1, 3, 5, 9]                                   # below, between and above the MFMA k = 4 padding
SHAPES = [(1, 1, 1), (3, 1, 4), (2, 2, 3), (4, 0, 3)]   # (nc, no, nv); (4, 0, 3) spin-orbital only
AO_COUNTS = [3, 1, 4, 0, 2, 5, 1, 3, 2]               # uneven; a single-AO atom, and one without AOs from natm = 5


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# ---- raw problems ---------------------------------------------------------------------
def _sym(rng, n, scale=1.0):
    m = rng.standard_normal((n, n)) * scale
    return 0.5 * (m + m.T)


@functools.lru_cache(maxsize=None)
def raw_problem(natm, shape, sa, correct, paramtype, seed=0):
    """Random non-orthogonal coefficients (different for the two spins), random symmetric Fock
    blocks, uneven atoms; the reference operands come from stda_ref (dense, atom-major)."""
    nc, no, nv = shape
    rng = np.random.default_rng(1000 * natm + 100 * nc + 10 * no + nv + seed)
    counts = AO_COUNTS[:natm]
    ao_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nao = int(ao_off[-1])
    nocc, nvir = [nc + no, nc], [nv, no + nv]
    nmo = nc + no + nv
    cprime = [0.4 * rng.standard_normal((nao, nmo)) for _ in range(2)]
    xyz = rng.standard_normal((natm, 3)) * 2.0
    dist = np.linalg.norm(xyz[:, None] - xyz[None], axis=2)
    gj, gk = ref.gamma(dist, rng.uniform(5.0, 9.5, natm), 0.2, paramtype)
    pr = dict(natm=natm, nc=nc, no=no, nv=nv, nocc=nocc, nvir=nvir, sa=bool(sa), si=no / 2, correct=bool(correct),
              dmax=0.5 / ref.HA2EV if correct else 0.0, sigk=0.1 / ref.HA2EV if correct else 1.0, gj=gj, gk=gk,
              qoo=[], qov=[], qvv=[], foo=[], fvv=[], hoo=[], hvv=[])
    for s in range(2):
        qoo, qov, qvv = ref.charges(cprime[s], ao_off, nocc[s])
        pr["qoo"].append(qoo); pr["qov"].append(qov); pr["qvv"].append(qvv)
        f, h = _sym(rng, nmo) + np.diag(np.arange(nmo) * 0.3), _sym(rng, nmo)
        pr["foo"].append(f[:nocc[s], :nocc[s]]); pr["fvv"].append(f[nocc[s]:, nocc[s]:])
        pr["hoo"].append(h[:nocc[s], :nocc[s]]); pr["hvv"].append(h[nocc[s]:, nocc[s]:])
    return dict(pr=pr, cprime=cprime, ao_off=ao_off, nao=nao)


def every_csf(pr):
    return np.concatenate([ref.to_triples(k, *lst, pr["nc"], pr["no"])
                           for k, lst in enumerate(ref.class_lists(pr["nc"], pr["no"], pr["nv"]))])


def random_list(pr, n, rng):
    """n CSFs in arbitrary order: distinct while the space has that many, repeated beyond."""
    pool = every_csf(pr)
    return pool[rng.choice(len(pool), size=n, replace=n > len(pool))]


class Device:
    """The operands of a raw problem on the device, built by xt_stda_charges / xt_stda_half."""

    def __init__(self, torch, lib, p):
        from xtddft_amd import _capi
        self.torch, self.L, self.capi = torch, lib, _capi
        pr = p["pr"]
        self.pr = pr
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.desc = _capi.XtStdaDesc(natm=pr["natm"], nocc_a=pr["nocc"][0], nvir_a=pr["nvir"][0], nocc_b=pr["nocc"][1],
                                     nvir_b=pr["nvir"][1], nc=pr["nc"], no=pr["no"], nv=pr["nv"],
                                     spin_adapted=int(pr["sa"]), si=pr["si"], correct=int(pr["correct"]),
                                     delta_max=pr["dmax"], sigma_k=pr["sigk"] if pr["correct"] else 0.0)
        self.ops = _capi.XtStdaOps()
        self.t = {}
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        gk, gj = up(pr["gk"]), up(pr["gj"])
        off = np.ascontiguousarray(p["ao_off"], dtype=np.int32)
        natm = pr["natm"]
        for s, tag in enumerate("ab"):
            o, v = pr["nocc"][s], pr["nvir"][s]
            nan = lambda n: torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda")
            t = dict(cp=up(p["cprime"][s]), q_oo=nan(o * o * natm), q_ov=nan(o * v * natm), q_vv=nan(v * v * natm),
                     k_ov=nan(o * v * natm), j_vv=nan(v * v * natm), f_oo=up(pr["foo"][s]), f_vv=up(pr["fvv"][s]),
                     h_oo=up(pr["hoo"][s]), h_vv=up(pr["hvv"][s]))
            _capi.check(lib.xt_stda_charges(ctypes.byref(self.desc), s, p["nao"], self._ip(off), t["cp"].data_ptr(),
                                            t["q_oo"].data_ptr(), t["q_ov"].data_ptr(), t["q_vv"].data_ptr(), self.st),
                        "xt_stda_charges")
            _capi.check(lib.xt_stda_half(ctypes.byref(self.desc), s, gk.data_ptr(), gj.data_ptr(), t["q_ov"].data_ptr(),
                                         t["q_vv"].data_ptr(), t["k_ov"].data_ptr(), t["j_vv"].data_ptr(), self.st),
                        "xt_stda_half")
            for name in _capi.STDA_OPS:
                setattr(self.ops, f"{name}_{tag}", t[name].data_ptr())
            self.t[s] = t
        self.keep = (gk, gj)

    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def block(self, s, name, shape):
        """A pair-major device block as the reference's atom-major array."""
        n = int(np.prod(shape))
        a = self.t[s][name][:n * self.pr["natm"]].cpu().numpy()
        return np.moveaxis(a.reshape(*shape, self.pr["natm"]), -1, 0)

    def matrix(self, csf):
        csf = np.ascontiguousarray(csf, dtype=np.int32)
        n = len(csf)
        a = self.torch.full((n, n), float("nan"), dtype=self.torch.float64, device="cuda")
        self.capi.check(self.L.xt_stda_matrix(ctypes.byref(self.desc), ctypes.byref(self.ops), n, self._ip(csf),
                                              a.data_ptr(), self.st), "xt_stda_matrix")
        return a.cpu().numpy()

    def diag(self, csf):
        csf = np.ascontiguousarray(csf, dtype=np.int32)
        n = len(csf)
        e = self.torch.full((2, n), float("nan"), dtype=self.torch.float64, device="cuda")
        self.capi.check(self.L.xt_stda_diag(ctypes.byref(self.desc), ctypes.byref(self.ops), n, self._ip(csf),
                                            e[0].data_ptr(), e[1].data_ptr(), self.st), "xt_stda_diag")
        return e.cpu().numpy()

    def select(self, csf_p, e_p, csf_n, e_n):
        csf_p, csf_n = np.ascontiguousarray(csf_p, dtype=np.int32), np.ascontiguousarray(csf_n, dtype=np.int32)
        ep, en = self.torch.from_numpy(e_p.copy()).cuda(), self.torch.from_numpy(e_n.copy()).cuda()
        w = self.torch.full((len(csf_n),), float("nan"), dtype=self.torch.float64, device="cuda")
        self.capi.check(self.L.xt_stda_select(ctypes.byref(self.desc), ctypes.byref(self.ops), len(csf_p),
                                              self._ip(csf_p), ep.data_ptr(), len(csf_n), self._ip(csf_n), en.data_ptr(),
                                              w.data_ptr(), self.st), "xt_stda_select")
        return w.cpu().numpy()


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


CONFIGS = [(natm, shape, sa, correct, pt) for natm in NATM for shape in SHAPES for sa in (0, 1)
           for correct in (0, 1) for pt in ("os", "cs") if not (sa and shape[1] == 0)]


@pytest.mark.parametrize("natm", NATM)
@pytest.mark.parametrize("shape", SHAPES)
def test_charges_and_half_match_the_restatement(torch, hiplib, natm, shape):
    for pt in ("os", "cs"):
        p = raw_problem(natm, shape, 0, 0, pt)
        d, pr = Device(torch, hiplib, p), p["pr"]
        for s in range(2):
            o, v = pr["nocc"][s], pr["nvir"][s]
            for name, want, shp in (("q_oo", pr["qoo"][s], (o, o)), ("q_ov", pr["qov"][s], (o, v)),
                                    ("q_vv", pr["qvv"][s], (v, v))):
                if o * v == 0 and name != "q_vv":
                    continue
                got = d.block(s, name, shp)
                assert np.abs(got - want).max() <= RTOL * max(np.abs(want).max(), 1e-300), (name, s)
            if o * v:
                want = np.einsum('nm,mia->nia', pr["gk"], pr["qov"][s])
                assert rel(d.block(s, "k_ov", (o, v)), want) < RTOL
            want = np.einsum('nm,mab->nab', pr["gj"], pr["qvv"][s])
            assert rel(d.block(s, "j_vv", (v, v)), want) < RTOL
        again = Device(torch, hiplib, p)     # xt_stda_charges / xt_stda_half once more: the same bits
        for s in range(2):
            for name in ("q_oo", "q_ov", "q_vv", "k_ov", "j_vv"):
                assert torch.equal(d.t[s][name], again.t[s][name]), (name, s)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"natm{c[0]}-{c[1][0]}{c[1][1]}{c[1][2]}-sa{c[2]}-c{c[3]}-{c[4]}")
def test_matrix_and_diag_match_the_restatement(torch, hiplib, config):
    """Lists of every length around the 16-wide tile, in arbitrary order; A and its transpose at
    RTOL; xt_stda_diag returns the bits of the diagonal of xt_stda_matrix; two calls, same bits."""
    p = raw_problem(*config)
    d, pr = Device(torch, hiplib, p), p["pr"]
    rng = np.random.default_rng(5)
    for n in (1, 15, 16, 17, 33):
        csf = random_list(pr, n, rng)
        want = ref.matrix(pr, csf)
        a = d.matrix(csf)
        scale = np.abs(want).max()
        err = np.abs(a - want).max() / scale
        print(f"{config} n={n}: rel err {err:.2e}, asym {np.abs(a - a.T).max() / scale:.2e}")
        assert err < RTOL
        assert np.abs(a - a.T).max() / scale < RTOL
        e, k = d.diag(csf)
        assert np.array_equal(e, np.diag(a))
        we, wk = ref.diag(pr, csf)
        assert np.abs(k - wk).max() <= RTOL * np.abs(wk).max()
        assert np.array_equal(a, d.matrix(csf)) and np.array_equal(np.stack([e, k]), d.diag(csf))


@pytest.mark.parametrize("sa", [0, 1])
@pytest.mark.parametrize("natm", [3, 9])
def test_matrix_on_one_spin_lists_and_empty_blocks(torch, hiplib, natm, sa):
    """An all-alpha list, an all-beta list, and a list with empty OV(aa) and CO(bb) blocks."""
    p = raw_problem(natm, (3, 1, 4), sa, 1, "os")
    d, pr = Device(torch, hiplib, p), p["pr"]
    pool = every_csf(pr)
    rng = np.random.default_rng(8)
    cv = pool[np.where((pool[:, 0] == 0) & (pool[:, 1] < pr["nc"]) | (pool[:, 0] == 1) & (pool[:, 2] >= pr["no"]))[0]]
    for name, lst in (("alpha", pool[pool[:, 0] == 0]), ("beta", pool[pool[:, 0] == 1]), ("cv only", cv)):
        lst = lst[rng.permutation(len(lst))]
        want = ref.matrix(pr, lst)
        err = rel(d.matrix(lst), want)
        print(f"natm {natm} sa {sa} {name} ({len(lst)}): rel err {err:.2e}")
        assert err < RTOL


SELECT_NP, SELECT_NN = (1, 7, 40), (1, 17, 300)


@functools.lru_cache(maxsize=None)
def select_case(natm, shape, paramtype, n_p, n_n):
    """Random P and N lists with E_N - E_P >= 0.05 Ha, and the reference's weights.  The seed is
    the first of 0, 1, 2, ... at which the REFERENCE has no weight within a factor 1.01 of the
    threshold (the device plays no part in the choice); the test asserts that condition.  The
    operands and B do not depend on spin_adapted or correct, so one case serves those variants."""
    pr = raw_problem(natm, shape, 0, 0, paramtype)["pr"]
    pool = every_csf(pr)
    for seed in range(200):
        rng = np.random.default_rng([seed, natm, n_p, n_n])
        csf_p = pool[rng.choice(len(pool), size=n_p, replace=n_p > len(pool))]
        csf_n = pool[rng.choice(len(pool), size=n_n, replace=n_n > len(pool))]
        e_p = rng.uniform(0.10, 0.30, n_p)
        e_n = rng.uniform(0.35, 1.50, n_n)
        want = ref.weights(pr, csf_p, e_p, csf_n, e_n)
        if np.exp(np.abs(np.log(want / ref.TP)).min()) > 1.01:
            break
    return csf_p, e_p, csf_n, e_n, want


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"natm{c[0]}-{c[1][0]}{c[1][1]}{c[1][2]}-sa{c[2]}-c{c[3]}-{c[4]}")
def test_select_matches_the_restatement(torch, hiplib, config):
    """The whole raw-entry grid (natm, shape, spin_adapted, correct, paramtype), each with
    nP in {1, 7, 40} x nN in {1, 17, 300}: w at RTOL, the selected set, the same bits twice."""
    natm, shape, sa, correct, pt = config
    p = raw_problem(*config)
    d = Device(torch, hiplib, p)
    worst = 0.0
    for n_p in SELECT_NP:
        for n_n in SELECT_NN:
            csf_p, e_p, csf_n, e_n, want = select_case(natm, shape, pt, n_p, n_n)
            assert (e_n[None, :] - e_p[:, None]).min() >= 0.05          # never the 1e-10 guard
            assert np.exp(np.abs(np.log(want / ref.TP)).min()) > 1.01   # no weight at the threshold
            w = d.select(csf_p, e_p, csf_n, e_n)
            err = np.abs(w - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err < RTOL, (n_p, n_n, err)
            assert np.array_equal(w >= ref.TP, want >= ref.TP)
            assert np.array_equal(w, d.select(csf_p, e_p, csf_n, e_n))
    print(f"{config}: worst rel err {worst:.2e}")


# ---- the driver on synthetic mean fields ---------------------------------------------------
SYN_ATOMS = dict(elements=["C", "H", "O", "H"], ao_atom=[0] * 5 + [1] + [2] * 4 + [3] * 2,
                 atom_coords=[[0.0, 0.1, 0.0], [1.9, 0.2, -0.3], [-0.4, 2.2, 0.5], [0.3, -0.8, 1.7]])
SYN_EMAX = 16.0     # eV: a real selection on both mean fields, every weight a factor > 1.012 from the threshold


def synthetic(kind):
    from xtddft_amd.synthetic import make_mf
    return make_mf(nao=12, nc=3, no=1, kind=kind, xctype="LDA", ngrid=8, naux=4)   # the smallest the helper takes here


def reference_run(mf, spinadapt, emax, cas, union, correct=False, nstates=6):
    eta = golden("stda_eta.json")["eta_eV"]
    xyz = np.asarray(SYN_ATOMS["atom_coords"], dtype=np.float64)
    dist = np.linalg.norm(xyz[:, None] - xyz[None], axis=2)
    off = np.searchsorted(SYN_ATOMS["ao_atom"], np.arange(5))
    pr, orbs, lo = ref.problem_from_mf(mf, spinadapt, emax, cas, correct, "os", [eta[e] for e in SYN_ATOMS["elements"]],
                                       off, dist)
    return ref.solve(pr, emax, union=union, nstates=nstates) + (pr, lo, orbs)


@pytest.mark.parametrize("emax,cas,union", [(SYN_EMAX, True, True), (SYN_EMAX, True, False), (SYN_EMAX, False, True),
                                            (SYN_EMAX, False, False), (None, True, True)])
@pytest.mark.parametrize("kind", ["RO", "U"])
def test_driver_matches_the_restatement(torch, kind, emax, cas, union):
    from xtddft_amd import OSsTDA
    mf = synthetic(kind)
    sa = kind == "RO"
    e, v, a, ps, counts, w, pr, lo, orbs = reference_run(mf, sa, emax, cas, union, correct=sa)
    if emax:   # conditions on the input: a real selection, no weight at the threshold
        assert 0 < (w >= ref.TP).sum() < w.size
        assert np.exp(np.abs(np.log(w / ref.TP)).min()) > 1.01
    x = OSsTDA(None, mf, spinadapt=sa, Emax=emax, cas=cas, union=union, correct=sa, nstates=6, diag="eigh",
               eta=golden("stda_eta.json")["eta_eV"], **SYN_ATOMS)
    e_ev, osc, rs, vv = x.kernel()
    assert (x.nc, x.no, x.nv, x.frozen_nc) == (pr["nc"], pr["no"], pr["nv"], lo)
    got = [(x.pscsfcv_a_i, x.pscsfcv_a_a), (x.pscsfov_a_i, x.pscsfov_a_a), (x.pscsfco_b_i, x.pscsfco_b_a),
           (x.pscsfcv_b_i, x.pscsfcv_b_a)]
    for k in range(4):
        assert np.array_equal(got[k][0], ps[k][0]) and np.array_equal(got[k][1], ps[k][1]), k
    assert (x.lcva, x.lova, x.lcob, x.lcvb) == tuple(len(q[0]) for q in ps)
    print(f"{kind} emax {emax} cas {cas} union {union}: dim {a.shape[0]}, A rel err {rel(x.A, a):.2e}")
    assert rel(x.A, a) < RTOL
    assert np.abs(x.e[:6] - e).max() < 1e-10
    assert np.abs(e_ev - e * ref.HA2EV).max() < 1e-8 and osc is None and np.all(rs == 0)
    if emax:
        assert rel(x.select_weights, w) < RTOL
    want_ds = ref.delta_s2_sa(v, ps) if sa else ref.delta_s2_so(v, ps, mf.get_ovlp(), *orbs, pr["nc"], pr["no"], pr["nv"])
    # eigenvectors of separated roots agree up to a sign; Delta<S^2> is quadratic in them
    assert np.abs(x.dS2 - want_ds).max() < 1e-8
    dip = np.random.default_rng(2).standard_normal((3, mf.nao, mf.nao))
    dip = dip + dip.transpose(0, 2, 1)
    f = ref.osc_str(e, v, ps, dip, *orbs, pr["nc"], pr["no"])
    assert np.abs(x.osc_str(dip) - f).max() < 1e-8 * max(1.0, np.abs(f).max())


@pytest.mark.parametrize("kind", ["RO", "U"])
def test_driver_davidson_matches_eigh(torch, kind):
    from xtddft_amd import OSsTDA
    mf = synthetic(kind)
    kw = dict(spinadapt=kind == "RO", Emax=None, nstates=4, eta=golden("stda_eta.json")["eta_eV"], **SYN_ATOMS)
    a = OSsTDA(None, mf, diag="eigh", **kw)
    a.kernel()
    b = OSsTDA(None, mf, diag="davidson", **kw)
    b.kernel()
    print(f"{kind}: davidson - eigh {np.abs(b.e[:4] - a.e[:4]).max():.2e} after {b.icyc} cycles")
    assert np.all(b.converged)
    assert np.abs(b.e[:4] - a.e[:4]).max() < b.conv_tol


# ---- the molecule --------------------------------------------------------------------------
def test_sutda_on_ch2o_reproduces_the_notebook(torch):
    from molecules import tda_meanfield
    from xtddft_amd import OSsTDA
    g = golden("stda_reference_outputs.json")["sutda_ch2o"]
    mf = tda_meanfield("CH2O_UKS")
    x = OSsTDA(mf.extra["qc_mol"], mf, spinadapt=False, nstates=12, eta=golden("stda_eta.json")["eta_eV"])
    e_ev, osc, rs, v = x.kernel()
    assert (x.nc, x.no, x.nv) == (5, 1, 9)
    assert x.A.shape == (g["dim"], g["dim"])
    assert (x.lcva, x.lova, x.lcob, x.lcvb) == (17, 3, 4, 17)
    assert x.pcsf_before_union == (g["pcsf_before_union"]["cv_a"], g["pcsf_before_union"]["cv_b"])
    assert x.pcsf_counts == tuple(g["pcsf"])
    assert (x.scsf_before_union[0], x.scsf_before_union[3]) == (g["scsf_before_union"]["cv_a"], g["scsf_before_union"]["cv_b"])
    print("roots", np.abs(e_ev - np.array(g["energy_eV"])).max(), "f", np.abs(osc - np.array(g["osc_str"])).max(),
          "dS2", np.abs(x.dS2 - np.array(g["deltaS2"])).max())
    assert np.abs(e_ev - np.array(g["energy_eV"])).max() < PRINT_TOL
    assert np.abs(osc - np.array(g["osc_str"])).max() < PRINT_TOL
    assert np.abs(x.dS2 - np.array(g["deltaS2"])).max() < PRINT_TOL
    assert np.all(rs == 0)
