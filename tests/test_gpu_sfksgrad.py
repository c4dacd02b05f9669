"""GPU: the XC response kernel ``xt_xc_resp`` (xtddft_amd/csrc/xt_xc_resp.hip) on random operands
against the ``einsum`` restatement ``tests/sfksgrad_ref.py``, ``DeviceEngine.fxc_response`` and
``qc.grad.grad_xc_pairs`` on CH2 / cc-pVDZ, and the collinear spin-flip TDA gradient on a UKS reference
(``xtddft_amd.grad.SFGradients``) against the restatement and against finite differences of device
energies on a grid frozen in space.

Raw calls are compared elementwise inside (nao + 32) 2^-53 S, S being the same expression with every
term replaced by its absolute value (``sfksgrad_ref.resp_arrays``): nao roundings in a dot product, at
most 16 in the fxc contraction and at most 5 in b; FMA contraction only lowers the count.
Translational and rotational sums do not vanish on a frozen grid and are printed, not asserted."""
import numpy as np
import pytest

import grad_ref as R
import sfksgrad_ref as SK
from xtddft_amd import _capi, qc
from xtddft_amd.grad import sf_amplitude
from xtddft_amd.qc import grad as G
from xtddft_amd.qc import xc as _xc
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"      # bent, unequal bonds, in the yz plane (Angstrom)
SF = {-1: SF_TDA_down, 1: SF_TDA_up}
GRIDS = (1, 63, 64, 65, 300)     # below, at and above one 64-point block, and several blocks with a remainder
NAOS = (1, 5, 64, 65, 130)       # rows shorter than, equal to and longer than one pass of a wave (128 AOs), odd and even


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# --------------------------------------------------------------------------- the kernel
def operands(ng, nao, gga, seed):
    """ao (4, G, nao), c (2, G, nao), fxc (2, nc, 2, nc, G) symmetric in (s k, s' k'), w (G,) of both signs."""
    rng = np.random.default_rng(seed)
    nc = 4 if gga else 1
    f = rng.standard_normal((2 * nc, 2 * nc, ng))
    f = (f + f.transpose(1, 0, 2)).reshape(2, nc, 2, nc, ng)
    return rng.standard_normal((4, ng, nao)), rng.standard_normal((2, ng, nao)), f, rng.standard_normal(ng)


def raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=0, want=("rho1", "wv", "b"), nan_planes=False):
    """One xt_xc_resp call with every operand in a buffer whose rows are at least ``pad`` doubles
    longer than they need to be (the padding NaN on the inputs; on the outputs it must stay NaN).
    An even ``pad`` gives even AO-row and plane strides (every row 16-byte aligned: the vector path,
    with a one-element tail when nao is odd), an odd one odd strides (the element path).  Returns
    {name: array} of the wanted outputs."""
    dv = torch.device("cuda:0")
    nc = 4 if gga else 1
    ng, nao = c.shape[1], c.shape[2]
    ld = nao + pad
    ld += (ld + pad) % 2                                   # the parity of pad
    ldao, ldc, ldb, ldg, ldo = ld, ld, ld, ng + pad, ng + pad
    ao_plane = ng * ldao + pad
    ao_plane += (ao_plane + pad) % 2
    assert ldao % 2 == pad % 2 and ao_plane % 2 == pad % 2 and ao_plane >= ng * ldao + pad
    nan = float("nan")

    def buf(shape):
        return torch.full(shape, nan, dtype=torch.float64, device=dv)

    def t(x):
        return torch.as_tensor(np.ascontiguousarray(x), device=dv)
    d_ao = buf((4 * ao_plane,))
    planes = 4 if (gga or not nan_planes) else 1           # nan_planes: LDA leaves planes 1..3 NaN
    for k in range(planes):
        d_ao[k * ao_plane:k * ao_plane + ng * ldao].view(ng, ldao)[:, :nao] = t(ao[k])
    d_c = buf((2, ng, ldc))
    d_c[:, :, :nao] = t(c)
    d_f = buf((2 * nc * 2 * nc, ldg))
    d_f[:, :ng] = t(fxc.reshape(-1, ng))
    d_w = t(w)
    d_rho, d_wv, d_b = buf((2, 4, ldo)), buf((2, 4, ldo)), buf((2, ng, ldb))
    rc = hiplib.xt_xc_resp(ng, nao, _capi.XC["GGA" if gga else "LDA"], d_ao.data_ptr(), ao_plane, ldao,
                           d_c.data_ptr(), ldc, d_f.data_ptr(), ldg, d_w.data_ptr(),
                           d_rho.data_ptr() if "rho1" in want else None, d_wv.data_ptr() if "wv" in want else None,
                           ldo, d_b.data_ptr() if "b" in want else None, ldb, None)
    _capi.check(rc, "xt_xc_resp")
    torch.cuda.synchronize()
    out = {}
    for name, arr, n in (("rho1", d_rho, ng), ("wv", d_wv, ng), ("b", d_b, nao)):
        a = arr.cpu().numpy()
        if name in want:
            assert np.isnan(a[..., n:]).all(), f"{name}: padding written"
            if name != "b" and not gga:
                assert np.isnan(a[:, 1:]).all(), f"{name}: LDA wrote planes 1..3"
                a = np.where(np.isnan(a), 0.0, a)
            out[name] = a[..., :n].copy()
        else:
            assert np.isnan(a).all(), f"{name}: a skipped output was written"
    return out


@pytest.mark.parametrize("nao", NAOS)
def test_kernel_against_restatement(torch, hiplib, nao):
    """Every grid size, both modes; even padding (two doubles: rows stay 16-byte aligned, the
    vector path) and odd padding (three: the element path), which must agree bit for bit."""
    worst = 0.0
    for ng in GRIDS:
        for gga in (False, True):
            ao, c, fxc, w = operands(ng, nao, gga, 1000 * nao + ng)
            ref, S = SK.resp_arrays(ao, c, fxc, w, gga)
            got2 = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=2)
            got3 = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=3)
            for name, r, s in zip(("rho1", "wv", "b"), ref, S):
                assert np.isfinite(got2[name]).all() and np.abs(r).max() > 0
                err = np.abs(got2[name] - r)
                bound = (nao + 32) * U * s
                worst = max(worst, float((err / np.where(s > 0, s, 1.0)).max()) / ((nao + 32) * U))
                assert (err <= bound).all(), (name, ng, nao, gga, float((err - bound).max()))
                assert got3[name].tobytes() == got2[name].tobytes(), (name, ng, nao, gga)
    print(f"nao = {nao}: largest |kernel - restatement| / ((nao + 32) 2^-53 S) = {worst:.3f} over grids {GRIDS}, LDA / GGA")


def test_null_outputs_leave_the_others_unchanged_and_calls_repeat(torch, hiplib):
    for gga in (False, True):
        ao, c, fxc, w = operands(300, 65, gga, 17)
        full = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=2)
        again = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=2)
        for name in full:
            assert full[name].tobytes() == again[name].tobytes()              # equal inputs, equal bits
        for skip in ("rho1", "wv", "b"):
            want = tuple(n for n in ("rho1", "wv", "b") if n != skip)
            part = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=3, want=want)
            for name in want:
                assert part[name].tobytes() == full[name].tobytes(), (gga, skip, name)
        only = raw_call(torch, hiplib, ao, c, fxc, w, gga, want=("wv",))          # what the gradient's second term asks
        assert only["wv"].tobytes() == full["wv"].tobytes()


def test_lda_mode_reads_plane_zero_only(torch, hiplib):
    """LDA mode with planes 1..3 of ao NaN and NaN behind every row of fxc gives the LDA answer bit
    for bit (the 2 x 2 kernel has no other unused part); the GGA answer differs."""
    ao, c, fxc4, w = operands(130, 65, True, 5)
    fxc = np.ascontiguousarray(fxc4[:, :1, :, :1])
    lda = raw_call(torch, hiplib, ao, c, fxc, w, False, pad=2)
    got = raw_call(torch, hiplib, ao, c, fxc, w, False, pad=2, nan_planes=True)
    for name in lda:
        assert np.isfinite(got[name]).all() and got[name].tobytes() == lda[name].tobytes()
    gga = raw_call(torch, hiplib, ao, c, fxc4, w, True, pad=2)
    assert np.abs(gga["b"] - lda["b"]).max() > 1e-3


def test_screened_points_give_exact_zeros(torch, hiplib):
    for gga in (False, True):
        ao, c, fxc, w = operands(200, 33, gga, 9)
        off = np.zeros(200, dtype=bool)
        off[[0, 5, 63, 64, 127, 199]] = True
        fxc[..., off] = 0.0
        got = raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=3)
        assert np.all(got["wv"][..., off] == 0.0) and np.all(got["b"][:, off] == 0.0)
        assert np.abs(got["wv"][:, 0][:, ~off]).min() > 0 and np.isfinite(got["b"]).all()
        assert np.abs(got["rho1"][:, 0][:, off]).min() > 0                     # rho1 itself is not screened


# --------------------------------------------------------------------------- CH2 / cc-pVDZ on the device
def _device_uks(mol, xc, grids=None):
    mf = qc.UKS(mol, xc=xc)
    if grids is not None:
        mf.grids = grids             # build() keeps a grid that is already set
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


def _device_states(mf, isf, davidson=False, **kw):
    td = SF[isf](mf.to_meanfield(), method=2, davidson=davidson, **kw)
    td.kernel(nstates=2)
    return td


def _d0(mf):
    return np.asarray([mf.mo_coeff[s][:, mf.mo_occ[s] > 0] @ mf.mo_coeff[s][:, mf.mo_occ[s] > 0].T for s in range(2)])


def _xao(mf, td, root):
    s = (0, 1) if td.isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    return cv @ sf_amplitude(td, root) @ co.T


@pytest.fixture(scope="module")
def ch2(hiplib):
    """The molecule, its dense derivative ERIs and, per functional on one shared grid: the device
    UKS, the restatement's XC arrays, its Z-vector matrices, the dense collinear states."""
    mol = qc.M(CH2, basis="cc-pvdz", spin=2)
    assert mol.nao == 24
    return mol, R.deriv_eri(mol), {}


def _case(ch2, xc):
    mol, _, cache = ch2
    if xc not in cache:
        mf = _device_uks(mol, xc, cache[next(iter(cache))]["mf"].grids if cache else None)
        ao10 = cache[next(iter(cache))]["xa"].ao10 if cache else None
        cache[xc] = dict(mf=mf, xa=SK.xc_arrays(mf, ao10), mcache={}, td={})
    return cache[xc]


def _td(case, isf):
    if isf not in case["td"]:
        case["td"][isf] = _device_states(case["mf"], isf)
    return case["td"][isf]


def test_fxc_response_against_restatement_and_chunked(ch2, torch):
    """V^resp and wv of a symmetric random density pair on the level-3 grid.  The restatement gets
    the engine's own AO values and fxc, so that what is compared is the response (GEMMs and
    xt_xc_resp), not the evaluation of the functional or of the AOs, whose last bits differ between
    host and device; bound (nao + 32) 2^-53 S with S summed over the grid.  Then chunks of 10 007 and
    3 000 points against one chunk, 1e-13 relative."""
    case = _case(ch2, "b3lyp")
    mf, xa = case["mf"], case["xa"]
    eng = mf.device_engine
    n, ng = mf.mol.nao, mf.grids.size
    rng = np.random.default_rng(2)
    dm = rng.standard_normal((2, n, n)) * 0.1
    dm = dm + dm.transpose(0, 2, 1)
    fxc_dev = eng.fxc_ground(mf.make_rdm1()).cpu().numpy()
    assert eng.fxc_ground() is eng.fxc_ground(mf.make_rdm1())                        # evaluated once, kept
    print(f"fxc on the device against the host: max relative difference "
          f"{np.abs(fxc_dev - xa.fxc).max() / np.abs(xa.fxc).max():.2e}")
    ao10 = xa.ao10.copy()
    ao10[:4] = eng.ao.cpu().numpy()
    v_ref, wv_ref, s_v, s_wv = SK.vresp_xc(xa._replace(ao10=ao10, fxc=fxc_dev), dm)
    eng.fxc_chunk = ng
    st = {}
    whole = eng.fxc_response(dm, want=("v", "wv"), stats=st)
    assert st["chunks"] == 1
    v, wv = whole["v"], whole["wv"].cpu().numpy()
    ev, ewv = np.abs(v - v_ref), np.abs(wv - wv_ref)
    print(f"fxc_response ({ng} points): max|V| = {np.abs(v_ref).max():.3e}, max|V - restatement| = {ev.max():.2e}, "
          f"largest error / bound: V {float((ev / ((n + 32) * U * s_v)).max()):.3f}, "
          f"wv {float((ewv / np.where(s_wv > 0, (n + 32) * U * s_wv, 1.0)).max()):.3f}")
    assert np.abs(v_ref).max() > 1e-3 and np.abs(v - v.transpose(0, 2, 1)).max() <= 1e-14
    assert (ev <= (n + 32) * U * s_v).all() and (ewv <= (n + 32) * U * s_wv).all()
    try:
        for chunk in (10007, 3000):
            assert ng % chunk and chunk % 64
            eng.fxc_chunk = chunk
            st = {}
            part = eng.fxc_response(dm, want=("v", "wv"), stats=st)
            err = np.abs(part["v"] - v).max() / np.abs(v).max()
            print(f"chunk {chunk} ({st['chunks']} chunks): relative difference of V {err:.2e}")
            assert st["chunks"] == -(-ng // chunk) and err <= 1e-13
            assert np.abs(part["wv"].cpu().numpy() - wv).max() <= 1e-13 * np.abs(wv).max()
    finally:
        eng.fxc_chunk = None
    only = eng.fxc_response(dm, want=("wv",))
    assert set(only) == {"wv"} and torch.equal(only["wv"], eng.fxc_response(dm, want=("v", "wv"))["wv"])
    with pytest.raises(ValueError):
        eng.fxc_response(dm, want=("rho",))


def test_grad_xc_pairs_single_pair_and_additivity(ch2, torch):
    case = _case(ch2, "b3lyp")
    mf = case["mf"]
    eng = mf.device_engine
    d0 = _d0(mf)
    ground = G.grad_xc_device(mf, d0[0], d0[1])
    h0 = _xc.eval_xc_eff_torch(mf.xc, eng.rho(d0), deriv=1)[1] * eng.w
    one = G.grad_xc_pairs(mf, [(h0, d0)])
    scale = np.abs(ground).max()
    print(f"grad_xc_pairs: single pair against grad_xc_device {np.abs(one - ground).max() / scale:.2e}")
    assert np.abs(one - ground).max() <= 1e-13 * scale
    rng = np.random.default_rng(4)
    dm = rng.standard_normal(d0.shape) * 0.1
    h1 = torch.as_tensor(rng.standard_normal(tuple(h0.shape)), device=eng.dev) * eng.w
    a, b = G.grad_xc_pairs(mf, [(h0, d0)]), G.grad_xc_pairs(mf, [(h1, dm)])
    both = G.grad_xc_pairs(mf, [(h0, d0), (h1, dm)], chunk=10007)
    s = max(np.abs(a).max(), np.abs(b).max())
    print(f"grad_xc_pairs: additivity {np.abs(both - (a + b)).max() / s:.2e}")
    assert np.abs(b).max() > 1e-6 and np.abs(both - (a + b)).max() <= 1e-13 * s
    sym = G.grad_xc_pairs(mf, [(h1, (dm + dm.transpose(0, 2, 1)) * 0.5)])      # the densities are symmetrised
    assert np.abs(sym - b).max() <= 1e-13 * s


CASES = [("b3lyp", -1, 1), ("b3lyp", -1, 2), ("b3lyp", 1, 1), ("bhandhlyp", -1, 1), ("bhandhlyp", -1, 2),
         ("bhandhlyp", 1, 1), ("pbe", -1, 1)]


@pytest.mark.parametrize("xc,isf,state", CASES)
def test_sf_gradient_on_uks_against_restatement(ch2, xc, isf, state):
    """method = 2, dense route; hybrids and a pure GGA (hyb = 0: the J-only two-electron path)."""
    mol, ip, _ = ch2
    case = _case(ch2, xc)
    mf, td = case["mf"], _td(case, isf)
    e_ref, _ = SK.sf_states(mf, isf)
    assert np.abs(np.asarray(td.e)[:4] - e_ref[:4]).max() <= 1e-8               # the collinear A of the device
    gm = td.nuc_grad_method()
    g = gm.kernel(state=state)
    tm = dict(gm.timings)
    ref, S, parts = SK.sf_ks_grad(mf, sf_amplitude(td, state - 1), isf, ip, case["xa"], mcache=case["mcache"])
    Rc = mol.atom_coords()
    print(f"SF {isf:+d} state {state} on UKS {xc}: omega = {td.e[state - 1]:.6f}, max|g| = {np.abs(ref).max():.4e}, "
          f"max|g_xc| = {np.abs(parts['xc']).max():.3e}, max|G_xc[wv; D0]| = {np.abs(parts['xc_fxc']).max():.3e}, "
          f"max|device - restatement| = {np.abs(g - ref).max():.2e}, max|g_xc device - restatement| = "
          f"{np.abs(gm.de_xc - parts['xc']).max():.2e}, Z-vector {tm['zvector_cycles']} cycles, residual "
          f"{tm['zvector_residual']:.1e}; xc_response_s = {tm['xc_response_s']:.3f} ({tm['xc_response_calls']} calls), "
          f"grad_xc_s = {tm['grad_xc_s']:.3f}; sum_A g = {g.sum(axis=0)}, sum_A R x g = {np.cross(Rc, g).sum(axis=0)}")
    assert g.shape == (3, 3) and len(tm["buckets"]) > 0
    assert tm["zvector_residual"] <= 1e-10
    assert np.abs(g - ref).max() <= 1e-8
    if state == 1:
        assert td.nuc_grad_method().kernel(state=1, atmlst=[2]).tobytes() == g[2:3].tobytes()


@pytest.mark.parametrize("isf", [-1, 1])
def test_sf_gradient_against_device_frozen_grid_finite_differences(ch2, isf):
    """B3LYP, state 1, e_tot + omega from the device drivers with the undisplaced grid, one random
    direction: |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2), h = 2e-3 Bohr."""
    mol, _, cache = ch2
    case = _case(ch2, "b3lyp")
    mf, td = case["mf"], _td(case, isf)
    g = td.nuc_grad_method().kernel(state=1)
    u = R.random_direction(mol.natm, 3)
    if "fd" not in case:
        case["fd"] = {sg * s: _device_uks(R.displaced(mol, u, sg * s), "b3lyp", mf.grids)
                      for s in (2 * H_FD, H_FD, H_FD / 2) for sg in (1, -1)}
    fd = case["fd"]
    x0 = _xao(mf, td, 0)

    def energy(s):
        m = fd[s]
        assert m.grids is mf.grids
        t = _device_states(m, isf)
        k, ov = R.follow(mf.s1e, x0, np.asarray([_xao(m, t, r) for r in range(6)]))
        assert ov > 0.9, (s, ov)
        return m.e_tot + t.e[k]
    eps_e = max([mf.last_energy_change] + [m.last_energy_change for m in fd.values()])
    fine, coarse = R.richardson(energy, H_FD)
    lhs = abs(float((g * u).sum()) - fine)
    rhs = 10 * abs(fine - coarse) + 10 * 2 * eps_e / (H_FD / 2)
    print(f"SF {isf:+d} state 1 on UKS b3lyp: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = {lhs:.2e} "
          f"<= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs


@pytest.mark.parametrize("isf", [-1, 1])
def test_davidson_route_gives_the_dense_gradient(ch2, isf):
    """State 1 from Davidson amplitudes converged to a residual of 1e-8: the gradient differs from
    the dense route's by at most ten times the root's residual norm against the dense A."""
    case = _case(ch2, "b3lyp")
    mf, dense = case["mf"], _td(case, isf)
    td = _device_states(mf, isf, davidson=True, conv_tol=1e-14, tol_residual=1e-8, lindep=1e-20)
    assert bool(np.asarray(td.converged)[0])
    A = dense.A
    v = np.asarray(td.v)[:, 0]
    v = v / np.linalg.norm(v)
    resid = np.linalg.norm(A @ v - (v @ A @ v) * v)
    g = td.nuc_grad_method().kernel(state=1)
    diff = np.abs(g - dense.nuc_grad_method().kernel(state=1)).max()
    print(f"Davidson route SF {isf:+d} on UKS b3lyp: residual norm {resid:.2e}, max gradient difference {diff:.2e}")
    assert resid <= 1e-8
    assert diff <= 10 * resid
    td.converged = np.array([False, False])
    with pytest.raises(RuntimeError):
        td.nuc_grad_method().kernel(state=1)


# --------------------------------------------------------------------------- the UHF reference is untouched
def _section15_grad_elec(scf, x_ab, flip, device, tol=1e-10, max_cycle=500):
    """The spin-flip CIS gradient on a UHF reference written out without ``hyb`` and without the XC
    hook, from the same pieces of the package (device J / K, ``solve_zvector`` with its default
    response, one ``xt_grad_jk`` call of eight pairs): the recording the driver is compared with."""
    mol = scf.mol
    s = (1, 0) if flip else (0, 1)
    C = [scf.mo_coeff[s[0]], scf.mo_coeff[s[1]]]
    occ = [scf.mo_occ[s[0]], scf.mo_occ[s[1]]]
    f_ao = scf.get_hcore()[None] + np.asarray(scf._veff)
    oa, va, ob, vb = C[0][:, occ[0] > 0], C[0][:, occ[0] == 0], C[1][:, occ[1] > 0], C[1][:, occ[1] == 0]
    na, nb = oa.shape[1], ob.shape[1]
    fa, fb = C[0].T @ f_ao[s[0]] @ C[0], C[1].T @ f_ao[s[1]] @ C[1]
    ta, tb = -x_ab.T @ x_ab, x_ab @ x_ab.T
    dta, dtb, dx = oa @ ta @ oa.T, vb @ tb @ vb.T, vb @ x_ab @ oa.T
    xs, xa = (dx + dx.T) / 2, (dx - dx.T) / 2
    vj, vk = scf.get_jk(dm=np.asarray((dta, dtb, xs, xa)), hermi=0)
    kx = C[1].T @ (vk[2] + vk[3]) @ C[0]
    ga, gb = vj[0] + vj[1] - vk[0], vj[0] + vj[1] - vk[1]
    ra = 2.0 * (va.T @ ga @ oa + fa[na:, :na] @ ta.T - kx[nb:, na:].T @ x_ab)
    rb = 2.0 * (vb.T @ gb @ ob - tb @ fb[:nb, nb:].T + x_ab @ kx[:nb, :na].T)
    from xtddft_amd.grad import _SpinView
    za, zb, _, _ = G.solve_zvector(_SpinView(scf, s), ra, rb, tol, max_cycle)
    z = np.asarray([va @ za @ oa.T, vb @ zb @ ob.T])
    zs = (z + z.transpose(0, 2, 1)) * 0.5
    vjz, vkz = scf.get_jk(dm=zs, hermi=0)
    gz = (vjz[0] + vjz[1])[None] - vkz
    wa, wb = np.zeros_like(fa), np.zeros_like(fb)
    wa[:na, :na] = fa[:na, :na] + oa.T @ (ga + gz[0]) @ oa + ta @ fa[:na, :na] - x_ab.T @ kx[nb:, :na]
    wb[:nb, :nb] = fb[:nb, :nb] + ob.T @ (gb + gz[1]) @ ob
    wb[nb:, nb:] = tb @ fb[nb:, nb:].T - x_ab @ kx[nb:, :na].T
    wa[na:, :na] = za @ fa[:na, :na].T
    wb[nb:, :nb] = zb @ fb[:nb, :nb].T - 2.0 * x_ab @ kx[:nb, :na].T
    W = C[0] @ wa @ C[0].T + C[1] @ wb @ C[1].T
    pa, pb = zs[0] + dta, zs[1] + dtb
    d0a, d0b = oa @ oa.T, ob @ ob.T
    de = G.contract_1e(mol, G.hcore_generator(mol), G.get_ovlp(mol), d0a + d0b + pa + pb, W)
    da, db, tz = d0a + pa, d0b + pb, pa + pb
    terms = [G.jk_terms(1, 0, da + db, da + db), G.jk_terms(-1, 0, tz, tz), G.jk_terms(0, -1, da, da),
             G.jk_terms(0, 1, pa, pa), G.jk_terms(0, -1, db, db), G.jk_terms(0, 1, pb, pb),
             G.jk_terms(0, -2, xs, xs), (0.0, 2.0, xa - xa.T, xa)]
    return de + G.grad_jk_device(mol, terms, device)


@pytest.mark.parametrize("isf", [-1, 1])
def test_uhf_reference_gradient_is_unchanged(ch2, isf):
    mol = ch2[0]
    mf = qc.UHF(mol)
    mf.conv_tol, mf.conv_tol_grad, mf.max_cycle = 1e-12, 1e-9, 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    td = SF[isf](mf.to_meanfield(), method=0, davidson=False)
    td.kernel(nstates=2)
    gm = td.nuc_grad_method()
    assert not gm.is_ks
    for state in (1, 2):
        g = gm.kernel(state=state)
        rec = _section15_grad_elec(mf, sf_amplitude(td, state - 1), isf == 1, 0) + G.grad_nuc(mol)
        diff = np.abs(g - rec).max()
        print(f"UHF reference SF {isf:+d} state {state}: max|driver - recording| = {diff:.2e} (max|g| = {np.abs(g).max():.3e})")
        assert diff <= 1e-13
        assert "xc_response_s" not in gm.timings and "grad_xc_s" not in gm.timings
