"""GPU: the kernels ``xt_xc_resp_sf`` / ``xt_xc_rows`` (xtddft_amd/csrc/xt_xc_resp_sf.hip) on random
operands against ``einsum``, ``DeviceEngine.fxc_sf_response`` / ``rows_potential`` and the device
``mcol.sf_mc_kernel_grad`` on CH2 / cc-pVDZ, and the multicollinear spin-flip TDA gradient on a UKS
reference (``xtddft_amd.grad.SFU_gradient`` / ``SFD_gradient``) against the restatement
``tests/sfmcgrad_ref.py`` and against finite differences of device energies on a grid frozen in space.

Raw calls are compared elementwise inside (nao + 16) 2^-53 S, S being the same expression with every
term replaced by its absolute value: nao roundings in a dot product, at most 5 in the contraction with
fxc_sf and at most 5 in b; FMA contraction only lowers the count."""
import numpy as np
import pytest

import grad_ref as R
import sfksgrad_ref as SK
import sfmcgrad_ref as MC
from test_gpu_sfksgrad import operands as resp_operands
from test_gpu_sfksgrad import raw_call as resp_raw_call
from xtddft_amd import _capi, mcol, qc
from xtddft_amd.grad import SFD_gradient, SFU_gradient, sf_amplitude
from xtddft_amd.sf_tda import SF_TDA_down, SF_TDA_up

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
H_FD = 2e-3
CH2 = "C 0 0 0; H 0 0.93 0.55; H 0 -0.99 0.62"
SF = {-1: SF_TDA_down, 1: SF_TDA_up}
GRAD = {-1: SFD_gradient, 1: SFU_gradient}
GRIDS = (1, 63, 64, 65, 300)
NAOS = (1, 5, 64, 65, 130)
SAMPLES = 20


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# --------------------------------------------------------------------------- the kernels
def operands(ng, nao, gga, seed):
    """ao (4, G, nao), c (G, nao), fxc_sf (nk, nk, G) symmetric, w (G,) of both signs."""
    rng = np.random.default_rng(seed)
    nk = 4 if gga else 1
    f = rng.standard_normal((nk, nk, ng))
    return rng.standard_normal((4, ng, nao)), rng.standard_normal((ng, nao)), f + f.transpose(1, 0, 2), rng.standard_normal(ng)


def resp_sf_ref(ao, c, f, w, gga):
    """((rho1 (4, G), wv (4, G), b (G, nao)), their S)."""
    nk = 4 if gga else 1
    G = c.shape[0]
    aa, ca = np.abs(ao), np.abs(c)
    rho1, s_rho = np.zeros((4, G)), np.zeros((4, G))
    rho1[0], s_rho[0] = np.einsum('gm,gm->g', ao[0], c), np.einsum('gm,gm->g', aa[0], ca)
    if gga:
        rho1[1:], s_rho[1:] = 2.0 * np.einsum('kgm,gm->kg', ao[1:4], c), 2.0 * np.einsum('kgm,gm->kg', aa[1:4], ca)
    wv, s_wv = np.zeros((4, G)), np.zeros((4, G))
    wv[:nk] = 2.0 * w * np.einsum('klg,lg->kg', f, rho1[:nk])
    s_wv[:nk] = 2.0 * np.abs(w) * np.einsum('klg,lg->kg', np.abs(f), s_rho[:nk])
    b, s_b = rows_ref(ao, wv[None], gga)
    s_b = rows_ref(aa, s_wv[None], gga)[0]
    return (rho1, wv, b[0]), (s_rho, s_wv, s_b[0])


def rows_ref(ao, wv, gga):
    """(b (nch, G, nao), S) of the weights wv (nch, 4, G)."""
    if gga:
        b = 0.5 * wv[:, 0][:, :, None] * ao[0][None] + np.einsum('ckg,kgm->cgm', wv[:, 1:], ao[1:4])
        s = 0.5 * np.abs(wv[:, 0])[:, :, None] * np.abs(ao[0])[None] + np.einsum('ckg,kgm->cgm', np.abs(wv[:, 1:]), np.abs(ao[1:4]))
    else:
        b, s = wv[:, 0][:, :, None] * ao[0][None], np.abs(wv[:, 0])[:, :, None] * np.abs(ao[0])[None]
    return b, s


class Buffers:
    """Padded device buffers: rows at least ``pad`` doubles longer than needed, the padding NaN.  An even
    ``pad`` gives even strides (the 16-byte path, with a one-element tail when nao is odd), an odd one odd
    strides (the element path)."""

    def __init__(self, torch, ng, nao, pad):
        self.torch, self.dv = torch, torch.device("cuda:0")
        self.ng, self.nao = ng, nao
        ld = nao + pad
        ld += (ld + pad) % 2
        self.ld, self.ldg = ld, ng + pad
        self.ao_plane = ng * ld + pad
        self.ao_plane += (self.ao_plane + pad) % 2
        assert ld % 2 == pad % 2 and self.ao_plane % 2 == pad % 2 and self.ao_plane >= ng * ld + pad

    def nan(self, shape):
        return self.torch.full(shape, float("nan"), dtype=self.torch.float64, device=self.dv)

    def t(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x), device=self.dv)

    def ao(self, ao, planes=4):
        d = self.nan((4 * self.ao_plane,))
        for k in range(planes):
            d[k * self.ao_plane:k * self.ao_plane + self.ng * self.ld].view(self.ng, self.ld)[:, :self.nao] = self.t(ao[k])
        return d

    def rows(self, x):                       # (..., G, nao) -> padded rows
        d = self.nan(tuple(x.shape[:-1]) + (self.ld,))
        d[..., :self.nao] = self.t(x)
        return d

    def planes(self, x):                     # (..., G) -> padded planes
        d = self.nan(tuple(x.shape[:-1]) + (self.ldg,))
        d[..., :self.ng] = self.t(x)
        return d


def raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=0, want=("rho1", "wv", "b"), nan_planes=False):
    ng, nao = c.shape
    B = Buffers(torch, ng, nao, pad)
    d_ao = B.ao(ao, 4 if (gga or not nan_planes) else 1)
    d_c, d_f, d_w = B.rows(c), B.planes(f.reshape(-1, ng)), B.t(w)
    d_rho, d_wv, d_b = B.nan((4, B.ldg)), B.nan((4, B.ldg)), B.nan((ng, B.ld))
    rc = hiplib.xt_xc_resp_sf(ng, nao, _capi.XC["GGA" if gga else "LDA"], d_ao.data_ptr(), B.ao_plane, B.ld,
                              d_c.data_ptr(), B.ld, d_f.data_ptr(), B.ldg, d_w.data_ptr(),
                              d_rho.data_ptr() if "rho1" in want else None, d_wv.data_ptr() if "wv" in want else None,
                              B.ldg, d_b.data_ptr() if "b" in want else None, B.ld, None)
    _capi.check(rc, "xt_xc_resp_sf")
    torch.cuda.synchronize()
    out = {}
    for name, arr, n in (("rho1", d_rho, ng), ("wv", d_wv, ng), ("b", d_b, nao)):
        a = arr.cpu().numpy()
        if name in want:
            assert np.isnan(a[..., n:]).all(), f"{name}: padding written"
            if name != "b" and not gga:
                assert np.isnan(a[1:]).all(), f"{name}: LDA wrote planes 1..3"
                a = np.where(np.isnan(a), 0.0, a)
            out[name] = a[..., :n].copy()
        else:
            assert np.isnan(a).all(), f"{name}: a skipped output was written"
    return out


def raw_rows(torch, hiplib, ao, wv, gga, pad=0, nan_planes=False):
    """b (nch, G, nao) of one xt_xc_rows call; ``nan_planes``: LDA with planes 1..3 of ao and of wv NaN."""
    nch, ng, nao = wv.shape[0], wv.shape[2], ao.shape[2]
    B = Buffers(torch, ng, nao, pad)
    d_ao = B.ao(ao, 4 if (gga or not nan_planes) else 1)
    wv = wv.copy()
    if nan_planes and not gga:
        wv[:, 1:] = np.nan
    d_wv = B.planes(wv.reshape(-1, ng))
    d_b = B.nan((nch, ng, B.ld))
    rc = hiplib.xt_xc_rows(ng, nao, _capi.XC["GGA" if gga else "LDA"], nch, d_ao.data_ptr(), B.ao_plane, B.ld,
                           d_wv.data_ptr(), B.ldg, d_b.data_ptr(), B.ld, None)
    _capi.check(rc, "xt_xc_rows")
    torch.cuda.synchronize()
    a = d_b.cpu().numpy()
    assert np.isnan(a[..., nao:]).all(), "b: padding written"
    return a[..., :nao].copy()


@pytest.mark.parametrize("nao", NAOS)
def test_kernels_against_einsum(torch, hiplib, nao):
    """Every grid size, both modes, nch = 1, 2, 4; even padding (the 16-byte path) and odd padding (the
    element path) agree bit for bit."""
    worst = 0.0
    for ng in GRIDS:
        for gga in (False, True):
            ao, c, f, w = operands(ng, nao, gga, 1000 * nao + ng)
            ref, S = resp_sf_ref(ao, c, f, w, gga)
            got2 = raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=2)
            got3 = raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=3)
            for name, r, s in zip(("rho1", "wv", "b"), ref, S):
                assert np.isfinite(got2[name]).all() and np.abs(r).max() > 0
                err = np.abs(got2[name] - r)
                bound = (nao + 16) * U * s
                worst = max(worst, float((err / np.where(s > 0, s, 1.0)).max()) / ((nao + 16) * U))
                assert (err <= bound).all(), (name, ng, nao, gga, float((err - bound).max()))
                assert got3[name].tobytes() == got2[name].tobytes(), (name, ng, nao, gga)
            wv = np.random.default_rng(ng + nao).standard_normal((4, 4, ng))
            if not gga:
                wv[:, 1:] = 0.0
            for nch in (1, 2, 4):
                r, s = rows_ref(ao, wv[:nch], gga)
                b2 = raw_rows(torch, hiplib, ao, wv[:nch], gga, pad=2)
                b3 = raw_rows(torch, hiplib, ao, wv[:nch], gga, pad=3)
                err = np.abs(b2 - r)
                worst = max(worst, float((err / np.where(s > 0, s, 1.0)).max()) / ((nao + 16) * U))
                assert np.isfinite(b2).all() and (err <= (nao + 16) * U * s).all(), (ng, nao, gga, nch)
                assert b3.tobytes() == b2.tobytes(), (ng, nao, gga, nch)
    print(f"nao = {nao}: largest |kernel - einsum| / ((nao + 16) 2^-53 S) = {worst:.3f} over grids {GRIDS}, LDA / GGA")


def test_null_outputs_repeats_lda_planes_and_zero_weights(torch, hiplib):
    for gga in (False, True):
        ao, c, f, w = operands(300, 65, gga, 17)
        full = raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=2)
        again = raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=2)
        for name in full:
            assert full[name].tobytes() == again[name].tobytes()              # equal inputs, equal bits
        for skip in ("rho1", "wv", "b"):
            want = tuple(n for n in ("rho1", "wv", "b") if n != skip)
            part = raw_resp_sf(torch, hiplib, ao, c, f, w, gga, pad=3, want=want)
            for name in want:
                assert part[name].tobytes() == full[name].tobytes(), (gga, skip, name)
        # zero weights at block edges: exact zeros in wv and b, from either entry
        off = np.zeros(300, dtype=bool)
        off[[0, 5, 63, 64, 127, 128, 299]] = True
        got = raw_resp_sf(torch, hiplib, ao, c, f, np.where(off, 0.0, w), gga, pad=3)
        assert np.all(got["wv"][:, off] == 0.0) and np.all(got["b"][off] == 0.0)
        assert np.abs(got["wv"][0][~off]).min() > 0 and np.abs(got["rho1"][0][off]).min() > 0
        wv = np.random.default_rng(3).standard_normal((2, 4, 300))
        wv[..., off] = 0.0
        if not gga:
            wv[:, 1:] = 0.0
        b = raw_rows(torch, hiplib, ao, wv, gga, pad=2)
        assert np.all(b[:, off] == 0.0) and np.abs(b[:, ~off]).min() > 0
        assert raw_rows(torch, hiplib, ao, wv, gga, pad=2).tobytes() == b.tobytes()
    # LDA reads plane 0 only and writes plane 0 only
    ao, c, f4, w = operands(130, 65, True, 5)
    f = np.ascontiguousarray(f4[:1, :1])
    lda = raw_resp_sf(torch, hiplib, ao, c, f, w, False, pad=2)
    got = raw_resp_sf(torch, hiplib, ao, c, f, w, False, pad=2, nan_planes=True)
    for name in lda:
        assert np.isfinite(got[name]).all() and got[name].tobytes() == lda[name].tobytes()
    assert np.abs(raw_resp_sf(torch, hiplib, ao, c, f4, w, True, pad=2)["b"] - lda["b"]).max() > 1e-3
    wv = np.random.default_rng(8).standard_normal((3, 4, 130))
    lda_b = raw_rows(torch, hiplib, ao, wv, False, pad=2)
    assert raw_rows(torch, hiplib, ao, wv, False, pad=2, nan_planes=True).tobytes() == lda_b.tobytes()
    assert np.isfinite(lda_b).all()


@pytest.mark.parametrize("gga", [False, True])
def test_rows_reproduce_the_third_pass_of_xt_xc_resp(torch, hiplib, gga):
    """``xt_xc_rows`` with two channels on the wv an ``xt_xc_resp`` call wrote gives that call's b bit for
    bit, on both alignment paths."""
    for ng, nao in ((300, 65), (64, 130), (65, 5)):
        ao, c, fxc, w = resp_operands(ng, nao, gga, 23)
        for pad in (2, 3):
            got = resp_raw_call(torch, hiplib, ao, c, fxc, w, gga, pad=pad)
            b = raw_rows(torch, hiplib, ao, got["wv"], gga, pad=pad)
            assert b.tobytes() == got["b"].tobytes(), (ng, nao, gga, pad)


# --------------------------------------------------------------------------- CH2 / cc-pVDZ on the device
def _device_uks(mol, xc, grids=None):
    mf = qc.UKS(mol, xc=xc)
    if grids is not None:
        mf.grids = grids
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


def _device_states(mf, isf, davidson=False, method=1, samples=SAMPLES, **kw):
    td = SF[isf](mf.to_meanfield(), method=method, davidson=davidson, collinear_samples=samples, **kw)
    td.kernel(nstates=2)
    return td


def _xao(mf, td, root):
    s = (0, 1) if td.isf == -1 else (1, 0)
    co = mf.mo_coeff[s[0]][:, mf.mo_occ[s[0]] > 0]
    cv = mf.mo_coeff[s[1]][:, mf.mo_occ[s[1]] == 0]
    return cv @ sf_amplitude(td, root) @ co.T


@pytest.fixture(scope="module")
def ch2(hiplib):
    mol = qc.M(CH2, basis="cc-pvdz", spin=2)
    assert mol.nao == 24
    return mol, R.deriv_eri(mol), {}


HOST_STRIDE = 32      # the host evaluates the restatement's tensor on every 32nd grid point (1 055 points)


def _mc_arrays(mf, xa):
    """The restatement's multicollinear arrays on the whole grid (20 samples).  On 33 734 points the host
    autograd of ``sfmcgrad_ref.mc_arrays`` takes about a minute per functional, so the whole grid is
    evaluated by the same function on the device, and the host evaluates every 32nd point, where both
    must agree to 1e-10 of the largest entry (the arrays are pointwise; 1e-10 is the bound the CPU tests
    hold the autograd of the kernel's derivative to)."""
    rho0 = MC.rho_of(xa.ao10, SK._d0(mf), xa.gga)
    mc = MC.mc_arrays(mf.xc, rho0, SAMPLES, device="cuda")
    host = MC.mc_arrays(mf.xc, rho0[:, :, ::HOST_STRIDE], SAMPLES)
    for name, d, h in (("fxc_sf", mc.fsf[..., ::HOST_STRIDE], host.fsf), ("kxc_sf", mc.kxc[..., ::HOST_STRIDE], host.kxc)):
        err = np.abs(d - h).max() / np.abs(h).max()
        print(f"{mf.xc}: restatement's {name}, device against host autograd on {h.shape[-1]} points: {err:.2e}")
        assert np.abs(h).max() > 0 and err <= 1e-10
    return mc


def _case(ch2, xc):
    """Per functional on one shared grid: the device UKS, the restatement's XC arrays and multicollinear
    arrays (``_mc_arrays``), its Z-vector matrices, the dense method = 1 states."""
    mol, _, cache = ch2
    if xc not in cache:
        first = cache[next(iter(cache))] if cache else None
        mf = _device_uks(mol, xc, first["mf"].grids if first else None)
        xa = SK.xc_arrays(mf, first["xa"].ao10 if first else None)
        cache[xc] = dict(mf=mf, xa=xa, mc=_mc_arrays(mf, xa), mcache={}, td={})
    return cache[xc]


def _td(case, isf):
    if isf not in case["td"]:
        case["td"][isf] = _device_states(case["mf"], isf)
    return case["td"][isf]


def test_engine_response_rows_and_kernel_gradient(ch2, torch):
    """``fxc_sf_response`` and ``rows_potential`` on the level-3 grid against the restatement fed the
    engine's own AO values and kernel, bound (nao + 16) 2^-53 S summed over the grid; two chunk lengths
    against one chunk to 1e-13 relative; the device ``sf_mc_kernel_grad`` against the host one on the
    engine's densities to 1e-8 of max|wv2|."""
    case = _case(ch2, "b3lyp")
    mf, xa = case["mf"], case["xa"]
    eng = mf.device_engine
    mfield = mf.to_meanfield()
    n, ng = mf.mol.nao, mf.grids.size
    rng = np.random.default_rng(2)
    x_s = rng.standard_normal((n, n)) * 0.1
    x_s = x_s + x_s.T
    kern = mcol.sf_mc_kernel(mfield, SAMPLES, device=0)
    kern_h = kern.cpu().numpy() if hasattr(kern, "cpu") else np.asarray(kern)
    print(f"fxc_sf on the device against the host restatement: max relative difference "
          f"{np.abs(kern_h - case['mc'].fsf).max() / np.abs(kern_h).max():.2e}")
    ao10 = xa.ao10.copy()
    ao10[:4] = eng.ao.cpu().numpy()
    xe = xa._replace(ao10=ao10)
    rho1_ref, wv1_ref, _, s_wv1 = MC.sf_weights(xe, MC.MCArrays(kern_h, None), x_s)
    v_ref, _ = MC.potential(xe, wv1_ref)
    s_v = MC.potential(xe._replace(ao10=np.abs(ao10)), s_wv1)[0]
    eng.fxc_chunk = ng
    try:
        st = {}
        whole = eng.fxc_sf_response(x_s, kern, want=("v", "wv", "rho1"), stats=st)
        assert st["chunks"] == 1
        v, wv = whole["v"], whole["wv"].cpu().numpy()
        ev, ewv = np.abs(v - v_ref), np.abs(wv - wv1_ref)
        print(f"fxc_sf_response ({ng} points): max|V_sf| = {np.abs(v_ref).max():.3e}, max|V_sf - restatement| = {ev.max():.2e}, "
              f"largest error / bound: V {float((ev / ((n + 16) * U * s_v)).max()):.3f}, "
              f"wv {float((ewv / np.where(s_wv1 > 0, (n + 16) * U * s_wv1, 1.0)).max()):.3f}")
        assert np.abs(v_ref).max() > 1e-4 and np.abs(v - v.T).max() <= 1e-14
        assert (ev <= (n + 16) * U * s_v).all() and (ewv <= (n + 16) * U * s_wv1).all()
        assert np.abs(whole["rho1"].cpu().numpy()[:4] - rho1_ref).max() <= 1e-12 * np.abs(rho1_ref).max()
        # rows_potential: three channels of random weights on the grid weights' scale
        w3 = torch.as_tensor(rng.standard_normal((3, 4, ng)), device=eng.dev) * eng.w
        p = eng.rows_potential(w3)
        w3h = w3.cpu().numpy()
        for ch in range(3):
            r = MC.potential(xe, w3h[ch])[0]
            s = MC.potential(xe._replace(ao10=np.abs(ao10)), np.abs(w3h[ch]))[0]
            assert (np.abs(p[ch] - r) <= (n + 16) * U * s).all(), ch
        for chunk in (10007, 3000):
            assert ng % chunk and chunk % 64
            eng.fxc_chunk = chunk
            st = {}
            part = eng.fxc_sf_response(x_s, kern, want=("v", "wv"), stats=st)
            err = np.abs(part["v"] - v).max() / np.abs(v).max()
            errp = np.abs(eng.rows_potential(w3) - p).max() / np.abs(p).max()
            print(f"chunk {chunk} ({st['chunks']} chunks): relative difference of V_sf {err:.2e}, of the row potentials {errp:.2e}")
            assert st["chunks"] == -(-ng // chunk) and err <= 1e-13 and errp <= 1e-13
            assert np.abs(part["wv"].cpu().numpy() - wv).max() <= 1e-13 * np.abs(wv).max()
    finally:
        eng.fxc_chunk = None
    with pytest.raises(ValueError):
        eng.fxc_sf_response(x_s, kern, want=("rho",))
    with pytest.raises(ValueError):
        eng.rows_potential(torch.zeros((5, 4, ng), dtype=torch.float64, device=eng.dev))
    # the kernel's density derivative: device against host at the same densities, every grid point
    rho0 = mcol.ground_state_rho(mfield, eng.dev)
    r1 = whole["rho1"][:4]
    q_d, dq_d = mcol.sf_mc_kernel_grad(mfield, r1, SAMPLES, device=0)
    q_d, dq_d = _host(q_d), _host(dq_d)
    sub = slice(None)
    r1h = r1.cpu().numpy()
    q_h, dq_h = mcol.sf_mc_kernel_grad(MC_fake(mf.xc), r1h[:, sub], SAMPLES, rho=rho0.cpu().numpy()[:, :, sub])
    w = eng.w.cpu().numpy()
    wv2_d, wv2_h = dq_d[:, :, sub] * w[sub], dq_h * w[sub]
    q_k = 2.0 * np.einsum('xg,xyg,yg->g', r1h, kern_h, r1h)
    err = np.abs(wv2_d - wv2_h).max() / np.abs(wv2_h).max()
    errq = np.abs(w * (q_d - q_k)).max() / np.abs(w * q_k).max()
    print(f"sf_mc_kernel_grad on the device ({wv2_h.shape[-1]} points): max|wv2| = {np.abs(wv2_h).max():.3e}, "
          f"device against host {err:.2e} of it; its scalar against the contraction of "
          f"sf_mc_kernel {errq:.2e}")
    assert err <= 1e-8 and errq <= 1e-12


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def MC_fake(xc):
    import types
    return types.SimpleNamespace(xc=xc, xctype=qc.xc.xc_type(xc), fxc_sf_mc=None, extra={}, mo_coeff=None, mo_occ=None,
                                 grids=types.SimpleNamespace(ao=None))


CASES = [("b3lyp", -1, 1), ("b3lyp", -1, 2), ("b3lyp", 1, 1), ("bhandhlyp", -1, 1), ("pbe", -1, 1), ("svwn", -1, 1)]


@pytest.mark.parametrize("xc,isf,state", CASES)
def test_mc_gradient_against_restatement(ch2, xc, isf, state):
    """method = 1, dense route, 20 samples: hybrids, a pure GGA (no K anywhere) and the LDA path."""
    mol, ip, _ = ch2
    case = _case(ch2, xc)
    mf, td = case["mf"], _td(case, isf)
    e_ref, _ = MC.sf_mc_states(mf, isf, case["xa"], case["mc"])
    print(f"method = 1 roots, device against restatement: {np.abs(np.asarray(td.e)[:4] - e_ref[:4]).max():.2e}")
    assert np.abs(np.asarray(td.e)[:4] - e_ref[:4]).max() <= 1e-7
    gm = GRAD[isf](td, method=1, state=state)
    assert gm.collinear_samples == SAMPLES
    g = gm.kernel()
    tm = dict(gm.timings)
    ref, S, parts = MC.sf_mc_grad(mf, sf_amplitude(td, state - 1), isf, ip, case["xa"], case["mc"], mcache=case["mcache"])
    print(f"SF {isf:+d} state {state}, multicollinear, UKS {xc}: omega = {td.e[state - 1]:.6f}, max|g| = {np.abs(ref).max():.4e}, "
          f"max|2 G_xc[wv1; X_S]| = {np.abs(parts['xc_sf']).max():.3e}, max|G_xc[wv2; D0]| = {np.abs(parts['xc_k']).max():.3e}, "
          f"max|device - restatement| = {np.abs(g - ref).max():.2e}, max|g_xc device - restatement| = "
          f"{np.abs(gm.de_xc - parts['xc']).max():.2e}, Z-vector {tm['zvector_cycles']} cycles, residual "
          f"{tm['zvector_residual']:.1e}; mc_kernel_grad_s = {tm['mc_kernel_grad_s']:.3f}, xc_sf_response_s = "
          f"{tm['xc_sf_response_s']:.3f}, xc_response_s = {tm['xc_response_s']:.3f}, grad_xc_s = {tm['grad_xc_s']:.3f}")
    assert g.shape == (3, 3) and gm.de is g
    assert tm["zvector_residual"] <= 1e-10
    assert np.abs(g - ref).max() <= 1e-8
    if state == 1:
        assert GRAD[isf](td).kernel(atmlst=[2]).tobytes() == g[2:3].tobytes()


@pytest.mark.parametrize("isf", [-1, 1])
def test_method_2_through_the_new_classes_is_nuc_grad_method(ch2, isf):
    case = _case(ch2, "b3lyp")
    td = _device_states(case["mf"], isf, method=2, samples=None)
    a = td.nuc_grad_method().kernel(state=1)
    gm = GRAD[isf](td, method=2)
    b = gm.kernel()
    assert a.tobytes() == b.tobytes()
    assert "mc_kernel_grad_s" not in gm.timings and "xc_sf_response_s" not in gm.timings


@pytest.mark.parametrize("xc,isf", [("b3lyp", -1), ("b3lyp", 1), ("pbe", -1)])
def test_mc_gradient_against_device_frozen_grid_finite_differences(ch2, xc, isf):
    """State 1, e_tot + omega from the device drivers (method = 1, 20 samples) with the undisplaced grid,
    one random direction: |g.u - R(h, h/2)| <= 10 |R(h, h/2) - R(2h, h)| + 10 * 2 eps_E / (h/2)."""
    mol, _, cache = ch2
    case = _case(ch2, xc)
    mf, td = case["mf"], _td(case, isf)
    g = GRAD[isf](td).kernel()
    u = R.random_direction(mol.natm, 3)
    if "fd" not in case:
        case["fd"] = {sg * s: _device_uks(R.displaced(mol, u, sg * s), xc, mf.grids)
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
    print(f"SF {isf:+d} state 1, multicollinear, UKS {xc}: g.u = {float((g * u).sum()):+.12f}, FD = {fine:+.12f}, |diff| = "
          f"{lhs:.2e} <= {rhs:.2e} (Richardson spread {abs(fine - coarse):.2e}, eps_E = {eps_e:.1e})")
    assert lhs <= rhs


def test_davidson_route_and_sample_counts(ch2):
    """State 1 of spin-flip-down from Davidson amplitudes (50 samples by default) against the dense route
    run with 50 samples: at most ten times the root's residual norm apart; an unconverged root is
    refused; the gradient objects use the sample count of their solver path."""
    case = _case(ch2, "b3lyp")
    mf = case["mf"]
    dense = _device_states(mf, -1, samples=50)
    td = _device_states(mf, -1, davidson=True, samples=None, conv_tol=1e-14, tol_residual=1e-8, lindep=1e-20)
    assert bool(np.asarray(td.converged)[0])
    gd, gdense = SFD_gradient(td), SFD_gradient(dense)
    assert gd.collinear_samples == 50 and gdense.collinear_samples == 50
    assert SFD_gradient(_device_states(mf, -1, samples=None)).collinear_samples == 30
    v = np.asarray(td.v)[:, 0]
    v = v / np.linalg.norm(v)
    resid = np.linalg.norm(dense.A @ v - (v @ dense.A @ v) * v)
    diff = np.abs(gd.kernel() - gdense.kernel()).max()
    print(f"Davidson route, multicollinear SF -1 on UKS b3lyp: residual norm {resid:.2e}, max gradient difference {diff:.2e}")
    assert resid <= 1e-8
    assert diff <= 10 * resid
    td.converged = np.array([False, False])
    with pytest.raises(RuntimeError):
        SFD_gradient(td).kernel()
