"""Host checks of the range-separated gradients (no GPU): the export list, header and argument checks of
the C entry ``xt_grad_jk2_lr``; the 40-digit long-range reference of tests/rsh_ref.py against the two wrong
references it is there to tell apart, and at its limits in omega; the far-pair case; the restatement
``rsh_ref.uks_grad_rsh`` against finite differences of host CAM-B3LYP energies on a grid frozen in space;
and the doors: ``.Gradients()`` takes the range-separated hybrids, ``nuc_grad_method()`` keeps refusing them.

Frozen grid: every displaced SCF gets the undisplaced ``Grids`` object, as in tests/test_ksgrad_host.py."""
import math
import os

import numpy as np
import pytest

import grad_cases as gc
import grad_ref as R
import hint_ref
import ksgrad_ref as K
import rsh_ref
from xtddft_amd import _capi, qc
from xtddft_amd.grad import SFD_gradient, SFGradients, SFU_gradient
from xtddft_amd.grad_utda import UTDAGradients
from xtddft_amd.qc import grad as G
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up
from xtddft_amd.xtda import XTDA

H_FD = 2e-3       # Bohr
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # the bent geometry of tests/test_gpu_grad.py (Angstrom)


# --------------------------------------------------------------------------- the C entry
def test_exports_and_header():
    assert "xt_grad_jk2_lr" in _capi.EXPORTS
    assert _capi.ABI_VERSION == 8                      # a pure addition: no bump
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xtddft_amd.h")) as f:
        text = f.read()
    assert "int xt_grad_jk2_lr(" in text and "double omega);" in text.split("int xt_grad_jk2_lr(")[1][:700]
    assert callable(G.grad_jk_rsh) and callable(G.pair_lists)


def test_xt_grad_jk2_lr_rejects_bad_arguments_without_gpu(hiplib):
    """Every rejected call returns XT_ERR_ARG (-1) with a message that names the entry and the argument,
    before the first HIP call; the zero-size calls return 0; an empty list may be null; omega must be finite
    and > 0."""
    L = hiplib
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data

    def call(nbra=1, binfo=i, bprim=d, eb=d, bao=i, nket=1, kinfo=i, kprim=d, ek=d, kao=i, lbra=3, lket=2, nj=2,
             wj=d, pj=d, qj=d, nk=2, wk=d, pk=d, qk=d, nao=1, strip=1, natm=1, work=d, nwork=6, out=d, omega=0.33):
        return L.xt_grad_jk2_lr(nbra, binfo, bprim, eb, bao, nket, kinfo, kprim, ek, kao, lbra, lket, nj, wj, pj, qj,
                                nk, wk, pk, qk, nao, strip, natm, work, nwork, out, None, omega)

    def rejected(rc, *words):
        assert rc == -1, rc
        msg = L.xt_last_error()
        assert b"xt_grad_jk2_lr" in msg, msg
        for word in words:
            assert word.encode() in msg, msg
    for omega in (0.0, -0.33, math.nan, math.inf, -math.inf):
        rejected(call(omega=omega), "omega")
        rejected(call(omega=omega, nbra=0), "omega")            # refused even where nothing would be added
    for name in ("nbra", "nket", "nao", "natm", "nwork"):
        rejected(call(**{name: -1}), "negative size")
    rejected(call(strip=0), "strip")
    for lb, lk in ((-1, 2), (3, -1), (9, 0), (8, 7), (7, 8)):
        rejected(call(lbra=lb, lket=lk), "order")
    for bad in (-1, 9):
        rejected(call(nj=bad), "nj")
        rejected(call(nk=bad), "nk")
    rejected(call(nj=0, nk=0), "both zero")
    rejected(call(nj=0, nk=0, wj=None, pj=None, qj=None, wk=None, pk=None, qk=None), "both zero")
    rejected(call(wj=None), "null", "wj")
    rejected(call(wk=None), "null", "wk")
    for name in ("pj", "qj"):
        rejected(call(**{name: None}), "null", "pj or qj")
    for name in ("pk", "qk"):
        rejected(call(**{name: None}), "null", "pk or qk")
    for name in ("binfo", "bprim", "eb", "bao", "kinfo", "kprim", "ek", "kao", "work", "out"):
        rejected(call(**{name: None}), "null")
    rejected(call(nwork=5), "workspace")
    rejected(call(nket=5, strip=2, nwork=11), "workspace")        # 3 strips + 1: 12 doubles
    rejected(call(nket=5, strip=2**31 - 1, nwork=5), "workspace")  # no int overflow in the strip count
    # the gradient's own shape: no Coulomb pair, its pointers null; the checks that follow are reached
    rejected(call(nj=0, wj=None, pj=None, qj=None, nwork=5), "workspace")
    rejected(call(nk=0, wk=None, pk=None, qk=None, nwork=5), "workspace")
    assert call(nbra=0, binfo=None, out=None) == 0 and call(nket=0, kinfo=None) == 0      # nothing to add
    assert call(nbra=0, nk=0, wk=None, pk=None, qk=None) == 0
    assert call(natm=0, nj=0, wj=None, pj=None, qj=None, out=None) == 0
    # xt_grad_jk2 keeps its own name in its messages
    assert L.xt_grad_jk2(1, i, d, d, i, 1, i, d, d, i, 3, 2, 2, d, d, d, 2, d, d, d, 1, 1, 1, d, 5, d, None) == -1
    assert b"xt_grad_jk2:" in L.xt_last_error()


# --------------------------------------------------------------------------- the reference
SEPARATION_CASES = ("c10", "c21", "c32", "c43", "c54", "c76", "cth81", "cth108", "img_off", "fold", "nterm8")


@pytest.fixture(scope="module")
def kappa_lr():
    err, kap = rsh_ref.load_kappa()
    assert kap.shape == (gc.L_MAX + 1,) and np.all(kap == gc.kappa_from(err))      # the rule of make_grad_kappa.py
    return kap


@pytest.fixture(scope="module")
def refs():
    """Per case name: (call, long-range reference, its sabs, L per row, the two wrong references)."""
    out = {}

    def get(name):
        if name not in out:
            c, call = rsh_ref.far_case() if name == "far" else (gc.BY_NAME[name], gc.build(gc.BY_NAME[name]))
            ref, sabs, Lrow, _ = hint_ref.ref_grad(call, blocks=rsh_ref.grad_integrals_lr(call, rsh_ref.OMEGA))
            noscale = hint_ref.ref_grad(call, blocks=rsh_ref.grad_integrals_lr(call, rsh_ref.OMEGA, drop_scale=True))[0]
            full = hint_ref.ref_grad(call)[0]
            out[name] = (call, ref, sabs, Lrow, noscale, full)
        return out[name]
    return get


@pytest.mark.parametrize("name", SEPARATION_CASES + ("far",))
def test_the_reference_separates_the_bugs_it_is_for(refs, kappa_lr, name):
    """(a) the sqrt(a2 / alpha) scale dropped and (b) the full-range operator both differ from the long-range
    reference by more than the bound kappa_lr 2^-53 sabs, on every case: a condition on the inputs."""
    call, ref, sabs, Lrow, noscale, full = refs(name)
    live = Lrow >= 0
    bound = (kappa_lr[np.maximum(Lrow, 0)][:, None] * gc.U * sabs)[live]
    for tag, wrong in (("scale dropped", noscale), ("full range", full)):
        gap = (np.abs(wrong - ref)[live] / bound).max()
        print(f"{name}: {tag} is {gap:.3e} bounds away")
        assert gap > 1.0, (name, tag, gap)
    host = rsh_ref.host_grad_lr(call, rsh_ref.OMEGA)
    assert np.all(gc.units(host, ref, sabs, Lrow) <= kappa_lr[np.maximum(Lrow, 0)][:, None])


@pytest.mark.parametrize("name", ["c21", "c43"])
def test_limits_of_the_reference(name):
    """omega = 2^20: the long-range blocks are the full-range ones to 1e-9 relative (a2 / alpha = 1 - alpha /
    (alpha + w^2), alpha of order 1 here); omega = 2^-20: below 1e-5 of them, erf(w r) / r being at most 2 w / sqrt(pi)."""
    call = gc.build(gc.BY_NAME[name])
    full = hint_ref.grad_integrals(call)[0]
    big = rsh_ref.grad_integrals_lr(call, 2.0 ** 20)[0]
    small = rsh_ref.grad_integrals_lr(call, 2.0 ** -20)[0]
    scale = np.abs(full).max()
    assert scale > 0
    assert np.abs(big - full).max() <= 1e-9 * scale
    assert np.abs(small).max() <= 1e-5 * scale and np.abs(small).max() > 0
    # the host restatement agrees with ints.eri_quartet's own attenuation at an ordinary omega
    host = rsh_ref.host_integrals_lr(call, 0.33)[0]
    ref = rsh_ref.grad_integrals_lr(call, 0.33)[0]
    assert np.abs(host - ref).max() <= 1e-12 * np.abs(ref).max()


def test_far_pair_reaches_both_boys_regimes():
    """s and p shells, 1 and 3 primitives, two centres 20 Bohr apart: T' = a2 R^2 on both sides of 30 at
    omega = 0.33, so both branches of hint_boys run under attenuation; without it every quartet is above 30."""
    c, call = rsh_ref.far_case()
    assert sorted({b.la for b in c.bras} | {b.lb for b in c.bras}) == [0, 1]
    assert {int(r[2]) for r in call.binfo} == {3} and {int(r[1]) for r in call.kinfo} == {3, 9}
    bz, kz = call.bprim.reshape(-1, 4)[:, 3], call.kprim.reshape(-1, 4)[:, 3]
    assert np.all(bz == 0.0) and np.all(kz == 20.0)
    T = rsh_ref.boys_arguments(call, rsh_ref.OMEGA)
    print(f"far pair: a2 R^2 from {T.min():.2f} to {T.max():.2f} over {T.size} primitive quartets")
    assert T.min() < 30.0 < T.max() and np.sum(T < 30.0) >= 2 and np.sum(T > 30.0) >= 2
    p, s = call.bprim.reshape(-1, 4)[:, None, 0], call.kprim.reshape(-1, 4)[None, :, 0]
    assert (p * s / (p + s) * 400.0).min() > 30.0


# --------------------------------------------------------------------------- restated gradient
def run_uks(mol, xc, grids, conv_tol=1e-12):
    mf = qc.UKS(mol, xc=xc)
    mf.grids = grids                 # build() keeps a grid that is already set
    mf.conv_tol = conv_tol
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.kernel()
    assert mf.converged
    return mf


def test_restated_rsh_gradient_against_frozen_grid_finite_differences():
    """CH2 / 6-31G triplet, CAM-B3LYP on a coarse grid frozen in space, one random direction:
    |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr."""
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, 8)
    mf = run_uks(mol, "cam-b3lyp", grids)
    assert mf.omega == 0.33 and abs(mf.alpha - mf.hyb - 0.46) < 1e-12
    ip = R.deriv_eri(mol)
    g = rsh_ref.uks_grad_rsh(mf, ip)
    no_lr = K.uks_grad(mf, ip)[0]
    u = R.random_direction(mol.natm, 1)
    runs = {}
    for s in (2 * H_FD, H_FD, H_FD / 2):
        for sg in (1, -1):
            m = run_uks(R.displaced(mol, u, sg * s), "cam-b3lyp", grids)
            assert m.grids is grids
            runs[sg * s] = (m.e_tot, m.last_energy_change)
    eps_e = max([mf.last_energy_change] + [v[1] for v in runs.values()])
    fine, coarse = R.richardson(lambda s: runs[s][0], H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    miss = abs(float((no_lr * u).sum()) - fine)
    print(f"UKS cam-b3lyp ({grids.size} points): g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} "
          f"<= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e}); without the long-range "
          f"term |diff| = {miss:.2e}")
    assert lhs <= rhs
    assert miss > 10 * rhs                             # the rule sees a missing long-range term


# --------------------------------------------------------------------------- doors
@pytest.fixture(scope="module")
def host_scfs():
    mol = qc.M(CH2, basis="6-31g", spin=2)
    grids = K.coarse_grids(mol, 8)

    def make(build_mf, device=True):
        mf = build_mf(mol)
        if str(mf.xc).upper() != "HF":
            mf.grids = grids
        mf.max_cycle = 300
        mf.kernel()
        assert mf.converged
        mfield = mf.to_meanfield()
        if device:
            mf.to_device(0)          # records the device only; the SCF itself ran on the host
        return mf, mfield
    return mol, make


def _doors(mol, mfield):
    """{name: (maker of the TDA object, class its .Gradients() returns)} for every excited-state driver."""
    return {"xtda": (lambda: XTDA(mol, mfield, nstates=2, use_Davidson=False), UTDAGradients),
            "down 2": (lambda: SF_TDA_down(mfield, method=2, davidson=False), SFGradients),
            "up 2": (lambda: SF_TDA_up(mfield, method=2, davidson=False), SFGradients),
            "down 1": (lambda: SF_TDA_down(mfield, method=1, davidson=False), SFD_gradient),
            "up 1": (lambda: SF_TDA_up(mfield, method=1, davidson=False), SFU_gradient)}


@pytest.mark.parametrize("xc", ["cam-b3lyp", "wb97xd"])
def test_gradients_door_takes_the_range_separated_hybrids(host_scfs, xc):
    mol, make = host_scfs
    mf, mfield = make(lambda m: qc.UKS(m, xc=xc))
    assert mf.omega > 0
    gm = mf.Gradients()
    assert type(gm) is G.KSGradients and gm.grid_response is False
    with pytest.raises(NotImplementedError):
        gm.grid_response = True
    with pytest.raises(NotImplementedError) as err:
        mf.nuc_grad_method()
    assert "Gradients()" in str(err.value) and "range-separated" in str(err.value)
    with pytest.raises(NotImplementedError):
        G.check_ks_gradient_mf(mf)
    G.check_ks_gradient_mf(mf, allow_rsh=True)
    for name, (make_td, cls) in _doors(mol, mfield).items():
        td = make_td()
        g = td.Gradients(state=2)
        assert type(g) is cls and g.state == 2 and g.is_ks, name
        assert td.Gradients().state == 1
        with pytest.raises(NotImplementedError):                # the old doors stay shut
            td.nuc_grad_method()
    for cls, td in ((SFD_gradient, SF_TDA_down(mfield, method=1, davidson=False)),
                    (SFU_gradient, SF_TDA_up(mfield, method=1, davidson=False))):
        with pytest.raises(NotImplementedError):
            cls(td)
        assert cls(td, allow_rsh=True).method == 1


def test_gradients_door_on_what_nuc_grad_method_takes(host_scfs):
    """Global hybrids and Hartree-Fock: ``.Gradients()`` returns what ``nuc_grad_method()`` returns."""
    mol, make = host_scfs
    mf, mfield = make(lambda m: qc.UKS(m, xc="b3lyp"))
    assert type(mf.Gradients()) is G.KSGradients is type(mf.nuc_grad_method())
    for name, (make_td, cls) in _doors(mol, mfield).items():
        assert type(make_td().Gradients()) is cls, name
    hf, hffield = make(lambda m: qc.UHF(m))
    assert type(hf.Gradients()) is G.Gradients
    assert type(XTDA(mol, hffield, nstates=2, use_Davidson=False).Gradients()) is UTDAGradients
    assert type(SF_TDA_down(hffield, method=0, davidson=False).Gradients(state=3)) is SFGradients
    assert type(qc.UHF(mol).Gradients()) is G.Gradients           # UHF needs no device to construct
    for method in (1, 2):                                         # Hartree-Fock has method 0 only
        with pytest.raises(NotImplementedError):
            SF_TDA_down(hffield, method=method, davidson=False).Gradients()


def test_gradients_door_keeps_every_other_refusal(host_scfs):
    mol, make = host_scfs
    for build_mf in (lambda m: qc.ROKS(m, xc="cam-b3lyp"), lambda m: qc.UKS(m, xc="tpss"),
                     lambda m: qc.UKS(m, xc="cam-b3lyp", nlc=(6.0, 0.01)),
                     lambda m: qc.UKS(m, xc="cam-b3lyp").density_fit(), lambda m: qc.UKS(m, xc="cam-b3lyp").sfx2c1e()):
        with pytest.raises(NotImplementedError):
            build_mf(mol).to_device(0).Gradients()
    for build_mf in (lambda m: qc.UKS(m, xc="tpss"), lambda m: qc.UKS(m, xc="b3lyp", nlc=(6.0, 0.01)),
                     lambda m: qc.UKS(m, xc="cam-b3lyp").density_fit()):
        keep, field = make(build_mf)
        for name, (make_td, _) in _doors(mol, field).items():
            with pytest.raises(NotImplementedError):
                make_td().Gradients()
    loose = qc.UKS(mol, xc="cam-b3lyp").to_device(0)
    loose.eri_mode, loose.chol_tol = "cholesky", 1e-6             # the long-range factor is built at chol_tol too
    with pytest.raises(ValueError):
        loose.Gradients()
    with pytest.raises(NotImplementedError):                      # a Kohn-Sham mean field on the host
        qc.UKS(mol, xc="cam-b3lyp").Gradients()
    host, hfield = make(lambda m: qc.UKS(m, xc="cam-b3lyp"), device=False)
    for name, (make_td, _) in _doors(mol, hfield).items():
        with pytest.raises(NotImplementedError) as err:
            make_td().Gradients()
        assert "host" in str(err.value), name
    keep, field = make(lambda m: qc.UKS(m, xc="cam-b3lyp"))
    for cls in (SF_TDA_down, SF_TDA_up):                          # ALDA0 on a functional
        with pytest.raises(NotImplementedError) as err:
            cls(field, method=0, davidson=False).Gradients()
        assert "ALDA0" in str(err.value)
    # ROKS behind a TDA object
    rk, rfield = make(lambda m: qc.ROKS(m, xc="cam-b3lyp"))
    for name, (make_td, _) in _doors(mol, rfield).items():
        with pytest.raises(NotImplementedError):
            make_td().Gradients()


# --------------------------------------------------------------------------- plumbing
def test_omega_zero_is_todays_call(monkeypatch):
    """``grad_jk_lists(..., omega=0.0)`` and the default send the argument list of today to ``xt_grad_jk2``;
    omega > 0 sends the same list plus omega to ``xt_grad_jk2_lr``; the helpers form the two calls."""
    seen = []

    def fake(mol, device, strip, stats, name, make_call):
        seen.append(name)
        return np.zeros((mol.natm, 3))
    monkeypatch.setattr(G, "_launch_buckets", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    mol = R.shell_set("sp")
    p = np.eye(mol.nao)
    jl, kl = [(1.0, p, p)], [(-1.0, p, p), (0.5, p, p.T)]
    G.grad_jk_lists(mol, jl, kl)
    G.grad_jk_lists(mol, jl, kl, omega=0.0)
    G.grad_jk_lists(mol, [], kl, omega=0.33)
    assert seen == ["xt_grad_jk2", "xt_grad_jk2", "xt_grad_jk2_lr"]
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(ValueError):
            G.grad_jk_lists(mol, jl, kl, omega=bad)
    with pytest.raises(ValueError):
        G.grad_jk_lists(mol, [], [], omega=0.33)
    # the two calls of a range-separated hybrid, and each alone
    calls = []
    monkeypatch.setattr(G, "grad_jk_lists", lambda mol, j, k, device=0, strip=None, stats=None, omega=0.0:
                        calls.append((omega, [w for w, _, _ in j], [w for w, _, _ in k])) or np.zeros((mol.natm, 3)))
    G.grad_jk_rsh(mol, jl, kl, 0.33, 0.19, 0.65)
    assert calls == [(0.0, [1.0], [-0.19, 0.5 * 0.19]), (0.33, [], [-(0.65 - 0.19), 0.5 * (0.65 - 0.19)])]
    calls.clear()
    G.grad_jk_rsh(mol, [], kl, 0.2, 0.0, 1.0)                     # hyb = 0, no Coulomb pair: call 2 alone
    assert calls == [(0.2, [], [-1.0, 0.5])]
    calls.clear()
    G.grad_jk_rsh(mol, jl, kl, 0.2, 0.25, 0.25)                   # alpha = hyb: call 1 alone
    assert calls == [(0.0, [1.0], [-0.25, 0.125])]
    with pytest.raises(ValueError):
        G.grad_jk_rsh(mol, jl, kl, 0.0, 0.19, 0.65)
    # pair_lists: the spin-flip driver's (wj, wk, P, Q) pairs as two lists
    terms = [G.jk_terms(1, 0, p, p), G.jk_terms(0, -1, p, p), (0.0, 2.0, p, p)]
    j2, k2 = G.pair_lists(terms)
    assert [w for w, _, _ in j2] == [-1.0] and [w for w, _, _ in k2] == [1.0, 2.0]
    j3, k3 = G.pair_lists(G.ks_ground_terms(p, p, 1.0))
    assert len(j3) == 1 and len(k3) == 2
