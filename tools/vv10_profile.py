"""Device times of the VV10 (NLC) response kernel and its share of one A.x.

    python tools/vv10_profile.py --out profiles/vv10_response.json

Per-launch times from HIP events on the launch stream after a warm-up (median and minimum
of --repeat launches): xt_vv10_response on the NLC grid of CH2 / 6-31G (the end-to-end test's
grid and the front end's default grid, densities from a B3LYP ROKS run) and on a synthetic
cloud of 65 536 points, and the XC slot of xt_last_timings of the operator-level test case with
and without the NLC term.  The flop model next to each time is
pairs x GEN_FLOPS + 18 G^2 nz (generation of a pair's kernel values + its 3 x 3 block applied
to nz vectors); the generation count is per vector tile of 24.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, C, RHO_MIN = 4.8, 0.0093, 1e-8
GEN_FLOPS = 45      # R^2 (8), g_ij, g_ji (4), products and the reciprocal (~12), 1/x 1/y 1/s (5), phi..phi_xy (~16)
CH2 = "C 0 0 0; H 0 0.98934 -0.42079; H 0 -0.98934 -0.42079"


def time_response(torch, L, xyz, w, rho, gam, nz, repeat, warmup):
    G = len(rho)
    rng = np.random.default_rng(1)
    d = [torch.tensor(np.ascontiguousarray(x), device="cuda") for x in (xyz, w, rho, gam)]
    r1 = torch.tensor(rng.normal(size=(nz, G)), device="cuda")
    g1 = torch.tensor(rng.normal(size=(nz, G)) * gam, device="cuda")
    sums = torch.zeros((6, G), dtype=torch.float64, device="cuda")
    vr, vg = torch.empty_like(r1), torch.empty_like(r1)
    st = torch.cuda.current_stream().cuda_stream
    p = [x.data_ptr() for x in d]

    def ground():
        assert L.xt_vv10_ground(G, *p, B, C, RHO_MIN, 0, G, sums.data_ptr(), st) == 0

    def resp():
        assert L.xt_vv10_response(G, *p, B, C, RHO_MIN, sums.data_ptr(), nz, r1.data_ptr(), g1.data_ptr(), 0, G,
                                  vr.data_ptr(), vg.data_ptr(), st) == 0
    out = {}
    for name, fn in (("ground", ground), ("response", resp)):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name] = dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)))
    tiles = -(-nz // 24)
    flops = float(G) * G * (GEN_FLOPS * tiles + 18.0 * nz)
    out["response"].update(flops_model=flops, tflops_at_median=flops / out["response"]["ms_median"] * 1e-9)
    return dict(G=G, nz=nz, masked=int((rho <= RHO_MIN).sum()), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vv10_response.json")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback for a timing"
    from xtddft_amd import _capi
    from xtddft_amd.qc import M, ROKS, nlc
    L = _capi.lib()
    res = dict(device=torch.cuda.get_device_name(0), b=B, C=C, repeat=a.repeat, warmup=a.warmup, cases=[])
    mf = ROKS(M(CH2, basis="6-31g", charge=0, spin=2), "b3lyp")
    mf.kernel()
    dm = mf.make_rdm1().sum(0)
    for label, grid in (("ch2_631g_test_grid_14x26", (14, 26)), ("ch2_631g_default_grid_35x110", (35, 110))):
        g = nlc.gen_nlc_grids(mf.mol, *grid)
        rho, grad = nlc.density(np.asarray(mf.mol.eval_ao(g.coords, deriv=1)), dm)
        for nz in (1, 3, 20):
            r = time_response(torch, L, g.coords, g.weights, rho, (grad * grad).sum(0), nz, a.repeat, a.warmup)
            res["cases"].append(dict(label=label, **r))
            print(res["cases"][-1], flush=True)
    rng = np.random.default_rng(2)
    G = 65536
    xyz, w = rng.normal(size=(G, 3)) * 4.0, rng.uniform(0.01, 0.1, G)
    rho, gam = 10.0 ** rng.uniform(-4, 0, G), 10.0 ** rng.uniform(-6, 0, G)
    for nz in (1, 20):
        res["cases"].append(dict(label="synthetic_65536", **time_response(torch, L, xyz, w, rho, gam, nz, 5, 2)))
        print(res["cases"][-1], flush=True)
    # the NLC share of one A.x: the operator-level test case (nao 20, 300 NLC points), xc slot of xt_last_timings
    import ctypes
    import dataclasses
    from xtddft_amd.meanfield import Grid
    from xtddft_amd.operator import DeviceOperator
    from xtddft_amd.synthetic import make_mf, make_trial_vectors
    smf = make_mf(nao=20, nc=4, no=2, ngrid=500, xctype="GGA", hyb=0.2)
    grid = Grid(ao=rng.normal(size=(4, 300, 20)) * 0.25, weights=rng.uniform(0.05, 0.5, 300),
                coords=rng.normal(size=(300, 3)) * 2.0)
    share = {}
    for name, m in (("without_nlc", smf), ("with_nlc", dataclasses.replace(smf, nlc=True, nlc_pars=(B, C), nlc_grids=grid))):
        op = DeviceOperator(m, "XTDA")
        z = torch.tensor(make_trial_vectors(7, op.dim), device="cuda")
        t = []
        for i in range(a.warmup + a.repeat):
            op.apply(z)
            o = (ctypes.c_double * 4)()
            L.xt_last_timings(op._h, ctypes.addressof(o))
            if i >= a.warmup:
                t.append(list(o))
        t = np.median(np.asarray(t), axis=0)
        share[name] = dict(jk_ms=t[0], xc_ms=t[1], local_ms=t[2], total_ms=t[3])
    share["nlc_ms"] = share["with_nlc"]["xc_ms"] - share["without_nlc"]["xc_ms"]
    res["operator_case_nz7"] = share
    print(share, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
