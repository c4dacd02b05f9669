"""VV10 (NLC) on the device: xt_vv10_ground / xt_vv10_response against the NumPy restatement
of the second derivative of the stated energy (tests/vv10_ref.py, itself pinned to mpmath and the
complex step in tests/test_vv10_host.py), the operator-level term of xt_apply, and an end-to-end
molecule.  Parity with PySCF's get_vnlc_resp is not pinned (PySCF is not available)."""
import numpy as np
import pytest

import vv10_ref as ref

pytestmark = pytest.mark.gpu

B, C = 4.8, 0.0093
RTOL = 1e-12            # the project's sigma-parity bound, of max|output|
TILE = 64               # xt_vv10.hip: target points per block = source points per LDS tile
N_TILE = 24             # xt_vv10.hip: widest vector tile


def _cloud(G, seed):
    """G points, ~10 % below rho_min, a coincident pair, gamma nearly uniform on one half and
    spread over decades on the other."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(G, 3)) * 2.0
    w = rng.uniform(0.1, 1.0, G)
    rho = 10.0 ** rng.uniform(-3.0, 0.3, G)
    gamma = np.where(np.arange(G) % 2 == 0, 0.2 * (1 + 1e-3 * rng.normal(size=G)), 10.0 ** rng.uniform(-6, 0.5, G))
    if G > 1:
        rho[rng.random(G) < 0.1] = 3e-9
        xyz[G - 1] = xyz[0]
        rho[0] = 0.3
        rho[G - 1] = 0.7
    return xyz, w, rho, gamma


_REF = {}


def _reference(G, nz, seed=5):
    """The host reference of a (G, nz) case, computed once and shared."""
    key = (G, nz)
    if key not in _REF:
        xyz, w, rho, gamma = _cloud(G, seed + G)
        rng = np.random.default_rng(seed + 1000 + G)
        rho1 = rng.normal(size=(nz, G))
        gam1 = rng.normal(size=(nz, G)) * gamma
        t = ref.hess_terms(xyz, w, rho, gamma, B, C)
        sums = ref.ground_sums(xyz, w, rho, gamma, B, C)
        vr, vg = ref.hess_apply(xyz, w, rho, gamma, B, C, rho1, gam1, t=t)
        for a in (xyz, w, rho, gamma, rho1, gam1, sums, vr, vg):
            a.setflags(write=False)
        _REF[key] = dict(xyz=xyz, w=w, rho=rho, gamma=gamma, rho1=rho1, gam1=gam1, sums=sums, vr=vr, vg=vg)
    return _REF[key]


def _dev(torch, a):
    return torch.tensor(a, device="cuda")


def _windows(G):
    out = [(0, G), (G // 2, G // 2)]
    if G > 3:
        out.append((G // 3 + 1, G - G // 4 - 1))
    return out


# G: 1; below / at / above the 64-point target tile, which is also the source tile; several tiles, ragged
@pytest.mark.parametrize("G", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 8, 577])
def test_ground_sums_match_the_restatement(G):
    import torch
    from xtddft_amd import _capi
    L = _capi.lib()
    r = _reference(G, 3)
    d = {k: _dev(torch, r[k]) for k in ("xyz", "w", "rho", "gamma")}
    scale = np.abs(r["sums"]).max(axis=1, keepdims=True)
    scale[scale == 0.0] = 1.0          # G = 1: R = 0, so W, S1, S2 are exactly zero
    for i0, i1 in _windows(G):
        outs = []
        for _ in range(2):
            out = torch.full((6, G), 7.0, dtype=torch.float64, device="cuda")
            _capi.check(L.xt_vv10_ground(G, d["xyz"].data_ptr(), d["w"].data_ptr(), d["rho"].data_ptr(),
                                         d["gamma"].data_ptr(), B, C, ref.RHO_MIN, i0, i1, out.data_ptr(), None),
                        "xt_vv10_ground")
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1])
        got = outs[0]
        assert np.all(got[:, :i0] == 7.0) and np.all(got[:, i1:] == 7.0)      # only the window is written
        err = np.abs(got[:, i0:i1] - r["sums"][:, i0:i1]) / scale
        print(G, (i0, i1), err.max() if err.size else 0.0)
        assert np.all(err <= RTOL)
        masked = np.nonzero(r["rho"][i0:i1] <= ref.RHO_MIN)[0] + i0
        assert np.all(got[:, masked] == 0.0)


# nz: 1, 3, 20 and one above the widest vector tile (two tiles, the second ragged)
@pytest.mark.parametrize("nz", [1, 3, 20, N_TILE + 5])
@pytest.mark.parametrize("G", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 8, 577])
def test_response_matches_the_restatement(G, nz):
    import torch
    from xtddft_amd import _capi
    L = _capi.lib()
    r = _reference(G, nz)
    d = {k: _dev(torch, r[k]) for k in ("xyz", "w", "rho", "gamma", "sums", "rho1", "gam1")}
    scale_r, scale_g = np.abs(r["vr"]).max(), np.abs(r["vg"]).max()
    for i0, i1 in _windows(G):
        outs = []
        for _ in range(2):
            vr = torch.full((nz, G), 7.0, dtype=torch.float64, device="cuda")
            vg = torch.full((nz, G), 7.0, dtype=torch.float64, device="cuda")
            _capi.check(L.xt_vv10_response(G, d["xyz"].data_ptr(), d["w"].data_ptr(), d["rho"].data_ptr(),
                                           d["gamma"].data_ptr(), B, C, ref.RHO_MIN, d["sums"].data_ptr(), nz,
                                           d["rho1"].data_ptr(), d["gam1"].data_ptr(), i0, i1, vr.data_ptr(),
                                           vg.data_ptr(), None), "xt_vv10_response")
            torch.cuda.synchronize()
            outs.append((vr.cpu().numpy(), vg.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        for got, want, scale in ((outs[0][0], r["vr"], scale_r), (outs[0][1], r["vg"], scale_g)):
            assert np.all(got[:, :i0] == 7.0) and np.all(got[:, i1:] == 7.0)
            if i1 > i0 and scale > 0:
                err = np.abs(got[:, i0:i1] - want[:, i0:i1]).max() / scale
                print(G, nz, (i0, i1), err)
                assert err <= RTOL
            masked = np.nonzero(r["rho"][i0:i1] <= ref.RHO_MIN)[0] + i0
            assert np.all(got[:, masked] == 0.0)


# --------------------------------------------------------------------------- operator level
def _nlc_grid(mf, ngrid=300, seed=17):
    from xtddft_amd.meanfield import Grid
    rng = np.random.default_rng(seed)
    ao = rng.normal(size=(4, ngrid, mf.nao)) * 0.25
    coords = rng.normal(size=(ngrid, 3)) * 2.0
    w = rng.uniform(0.05, 0.5, ngrid)
    return Grid(ao=ao, weights=w, coords=coords)


def _restated_sigma(mf, grid, z):
    """C_occ^T V1 C_vir per spin channel, V1 = the restated AO response of the total
    first-order density matrix, in the solver's vector order [za | zb]."""
    ca, cb, oa, ob = mf.spin_occupations()
    coa, cva = ca[:, oa > 0], ca[:, oa == 0]
    cob, cvb = cb[:, ob > 0], cb[:, ob == 0]
    na = coa.shape[1] * cva.shape[1]
    dm0 = mf.make_rdm1().sum(0)
    rho0, grad0 = ref.np_density(grid.ao, dm0)
    t = ref.hess_terms(grid.coords, grid.weights, rho0, (grad0 * grad0).sum(0), B, C)
    out = np.empty_like(z)
    for k, zk in enumerate(z):
        za = zk[:na].reshape(coa.shape[1], cva.shape[1])
        zb = zk[na:].reshape(cob.shape[1], cvb.shape[1])
        d1 = coa @ za @ cva.T + cob @ zb @ cvb.T
        v1 = ref.response_ao(grid.ao, grid.coords, grid.weights, dm0, d1, B, C, t=t)
        out[k] = np.concatenate([(coa.T @ v1 @ cva).ravel(), (cob.T @ v1 @ cvb).ravel()])
    return out


# the chunked case caps the chunk budget at 64 KiB: 7 vectors then take five chunks of 64, 64, 64, 64, 44 points
@pytest.mark.parametrize("nz,chunked", [(1, False), (7, False), (7, True)])
@pytest.mark.parametrize("kind", ["RO", "U"])
def test_operator_adds_the_projected_response(kind, nz, chunked, monkeypatch):
    import dataclasses
    from xtddft_amd.operator import DeviceOperator
    from xtddft_amd.synthetic import make_mf, make_trial_vectors
    if chunked:
        monkeypatch.setenv("XT_CHUNK_BYTES", "65536")
    mf = make_mf(nao=20, nc=4, no=2, ngrid=500, xctype="GGA", hyb=0.2, kind=kind)
    op_kind = "XTDA" if kind == "RO" else "UTDA"
    grid = _nlc_grid(mf)
    O = mf.shape_info()["nocc_a"]
    if chunked:    # the rule of nlc_response: budget / (8 bytes x 4 planes x 2 channels x nz x O), floor 64
        per = max(64, 65536 // (8 * 4 * 2 * nz * O))
        assert -(-grid.ngrid // per) >= 3 and grid.ngrid % per != 0
    mf_nlc = dataclasses.replace(mf, nlc=True, nlc_pars=(B, C), nlc_grids=grid)
    op0 = DeviceOperator(mf, op_kind)
    op1 = DeviceOperator(mf_nlc, op_kind)
    z = make_trial_vectors(nz, op0.dim)
    s0, s1 = op0.apply(z), op1.apply(z)
    want = _restated_sigma(mf, grid, z)
    scale = np.abs(s1).max()
    err = np.abs((s1 - s0) - want).max() / scale
    print(kind, nz, chunked, "nlc/sigma", np.abs(want).max() / scale, "err", err)
    assert np.abs(want).max() > 1e-6 * scale          # the term is visible at this bound
    assert err <= RTOL
    if nz > 1:     # A is symmetric with the term
        g = z @ s1.T
        assert np.abs(g - g.T).max() <= RTOL * (np.abs(z) @ np.abs(s1).T).max()


# --------------------------------------------------------------------------- end to end
CH2 = "C 0 0 0; H 0 0.98934 -0.42079; H 0 -0.98934 -0.42079"      # 3B1: C-H 1.075 A, H-C-H 133.9 degrees
NLC_GRID = (14, 26)                                                # per atom: 3 x 364 points


def _ch2_scf(device):
    from xtddft_amd.qc import M, ROKS
    mf = ROKS(M(CH2, basis="6-31g", charge=0, spin=2), "b3lyp", nlc=(B, C))
    mf.nlc_grid = NLC_GRID
    if device:
        mf.to_device(0)
    mf.kernel()
    assert mf.converged
    return mf


def _host_arrays(mf):
    """The same MeanField with every device tensor copied to a NumPy array (the oracle is NumPy)."""
    import dataclasses

    def conv(x):
        if type(x).__module__.startswith("torch"):
            return x.cpu().numpy()
        if dataclasses.is_dataclass(x) and not isinstance(x, type) and type(x).__name__ == "Grid":
            return dataclasses.replace(x, **{f.name: conv(getattr(x, f.name)) for f in dataclasses.fields(x)})
        return x
    return dataclasses.replace(mf, **{f.name: conv(getattr(mf, f.name)) for f in dataclasses.fields(mf)
                                      if f.name != "extra"})


def test_ch2_b3lyp_vv10_end_to_end():
    """CH2 3B1 / 6-31G, B3LYP + VV10 (b, C) = (4.8, 0.0093), ROKS on the device: the SCF energy equals
    the host SCF's (1e-9 Ha, the bound of test_gpu_qc.py), X-TDA returns, every root's residual holds
    under a fresh xt_apply, and the roots are the lowest eigenvalues of the dense matrix assembled from
    the oracle's columns without NLC plus the restated NLC columns (1e-7 Ha, the bound of
    test_gpu_molecule.py for Davidson against dense diagonalisation).

    kernel() starts, as the reference does, from the nstates = 3 lowest orbital gaps.  In this C2v
    molecule the third dense root (0.29686 Ha) is dominated by the configuration of the fourth-lowest
    gap, in an irrep none of those three start vectors touches, so a 3-vector start converges to
    roots 1, 2 and 4 with or without NLC.  The comparison with the LOWEST dense eigenvalues is
    therefore made on a solve started from the six lowest gaps; kernel()'s own roots must each be
    an eigenvalue of the dense matrix."""
    import dataclasses
    from oracle import xtda as oxtda
    from xtddft_amd import XTDA
    host, dev = _ch2_scf(False), _ch2_scf(True)
    print("E host", host.e_tot, "E device", dev.e_tot)
    assert abs(dev.e_tot - host.e_tot) < 1e-9
    mf = dev.to_meanfield()
    assert mf.nlc and mf.nlc_pars == (B, C) and mf.nlc_grids.ngrid == 3 * NLC_GRID[0] * NLC_GRID[1]
    x = XTDA(mf.mol, mf, nstates=3)
    e = np.asarray(x.kernel())
    assert np.all(x.converged)
    # residuals with a fresh A.x, vectors back in the solver's order
    v = np.empty_like(x.v)
    v[x.order] = x.v
    s = x.operator().apply(np.ascontiguousarray(v.T))
    res = np.linalg.norm(s - e[:, None] * v.T, axis=1)
    print("roots", e, "residuals", res)
    assert np.all(res <= x.conv_tol)
    # dense reference: oracle A without the NLC response + the restated NLC columns
    mh = _host_arrays(mf)
    vind, hdiag = oxtda.gen_tda_operation(dataclasses.replace(mh, nlc=False))
    eye = np.eye(hdiag.size)
    a = vind(eye) + _restated_sigma(mh, mh.nlc_grids, eye)
    w = np.linalg.eigvalsh(0.5 * (a + a.T))
    w_plain = np.linalg.eigvalsh(vind(eye).T)
    w, w_plain = w[w > 1e-3], w_plain[w_plain > 1e-3]
    print("dense", w[:4], "shift by the NLC response", (w - w_plain)[:4])
    assert np.abs(a - a.T).max() < 1e-10 * np.abs(a).max()
    assert np.abs(w - w_plain)[:3].min() > 1e-6          # the NLC response is visible at the bound
    assert np.abs(e[:, None] - w[None, :]).min(axis=1).max() < 1e-7
    x6 = XTDA(mf.mol, mf, nstates=3)
    e6 = np.asarray(x6.Davidson(x0=x6.get_init_guess(mf, nstates=6)))
    print("roots from the six lowest gaps", e6)
    assert np.all(x6.converged)
    assert np.abs(e6 - w[:3]).max() < 1e-7
