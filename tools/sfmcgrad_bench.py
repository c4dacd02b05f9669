"""Device timing of the multicollinear spin-flip TDA gradient on a UKS reference
(``xtddft_amd.grad.SFD_gradient``, ``method = 1``; kernels ``xt_xc_resp_sf`` / ``xt_xc_rows`` next to
those of ``tools/sfksgrad_bench.py``) on the molecule of that tool: naphthalene+ / cc-pVDZ, UKS / B3LYP,
spin-flip-down state 1.

    python tools/sfmcgrad_bench.py [--molecule naphthalene+] [--xc b3lyp] [--out profiles/sfmcgrad_bench.json]

Recorded, from the second of two gradient evaluations: the split of the gradient's seconds, the
autograd pass of ``mcol.sf_mc_kernel_grad`` (``mc_kernel_grad_s``) and the spin-flip channel
(``xc_sf_response_s``) included.  On one grid chunk of the same data ``xt_xc_resp_sf`` and ``xt_xc_rows``
(two channels) are timed against the same arrays composed from torch operations, with the bytes each
side moves counted from the operations.  Recorded, not gated.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_resp_sf(torch, ao, c, f, w, gga):
    """rho1, wv = 2 w fxc_sf rho1 and b from torch passes over the G x nao planes."""
    nk = 4 if gga else 1
    rho1 = torch.stack([(ao[0] * c).sum(1)] + [2.0 * (ao[k] * c).sum(1) for k in range(1, nk)])
    wv = 2.0 * torch.einsum('klg,lg->kg', f, rho1) * w
    return rho1, wv, torch_rows(torch, ao, wv[None], gga)[0]


def torch_rows(torch, ao, wv, gga):
    nk = 4 if gga else 1
    out = []
    for ch in range(wv.shape[0]):
        h = wv[ch, :nk].clone()
        if gga:
            h[0] *= 0.5
        out.append((h[:, :, None] * ao[:nk]).sum(0))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--xc", default="b3lyp")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfmcgrad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import _capi, build, mcol
    from xtddft_amd.grad import SFD_gradient
    from xtddft_amd.qc import M, UKS
    from xtddft_amd.sf_tda import SF_TDA_down
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("sfmcgrad_bench needs the GPU: nothing is measured without one")
    spec = MOLECULES[a.molecule]
    mol = M(spec["atom"], basis=spec["basis"], charge=spec.get("charge", 0), spin=spec.get("spin", 0),
            unit=spec.get("unit", "Angstrom"))

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    t0 = sync()
    mf = UKS(mol, xc=a.xc)
    mf.conv_tol = 1e-10
    mf.max_cycle = 200
    mf.to_device(0).cholesky(1e-12)
    mf.kernel()
    scf_s = sync() - t0
    res = dict(molecule=spec.get("label", a.molecule), xc=a.xc, nao=mol.nao, natm=mol.natm, nshell=len(mol.shells),
               ngrid=int(mf.grids.size), device=torch.cuda.get_device_name(0), scf_converged=bool(mf.converged),
               e_tot=float(mf.e_tot), scf_s=scf_s)
    t0 = sync()
    td = SF_TDA_down(mf.to_meanfield(), method=1, davidson=True, conv_tol=1e-10, tol_residual=1e-6)
    td.kernel(nstates=2)
    res["tda"] = dict(seconds=sync() - t0, omega=[float(x) for x in np.asarray(td.e)[:2]],
                      converged=[bool(x) for x in np.asarray(td.converged)[:2]])
    gm = SFD_gradient(td, method=1, state=1)
    res["collinear_samples"] = gm.collinear_samples
    runs = []
    for _ in range(2):
        t0 = sync()
        de = gm.kernel()
        runs.append((sync() - t0, dict(gm.timings)))
    total_s, tm = runs[1]
    sx = tm["grad_xc_stats"]
    res["gradient"] = dict(
        total_s=total_s, warmup_total_s=runs[0][0], one_electron_s=tm["one_electron_s"],
        grad_jk_s=sum(b["ms"] for b in tm["buckets"]) * 1e-3, grad_jk_call_s=tm["grad_jk_s"],
        zvector_s=tm["zvector_s"], zvector_cycles=tm["zvector_cycles"], zvector_residual=tm["zvector_residual"],
        xc_response_s=tm["xc_response_s"], xc_response_calls=tm["xc_response_calls"],
        mc_kernel_grad_s=tm["mc_kernel_grad_s"], xc_sf_response_s=tm["xc_sf_response_s"],
        grad_xc_pairs_s=tm["grad_xc_s"], grad_xc_gemm_s=sx["gemm_s"], grad_xc_kernel_s=sx["grad_xc_s"],
        max_abs_g=float(np.abs(de).max()), max_abs_g_xc=float(np.abs(gm.de_xc).max()),
        sum_g=[float(x) for x in de.sum(axis=0)])

    # xt_xc_resp_sf / xt_xc_rows against the torch composition on one chunk of the grid
    eng = mf.device_engine
    n, ng = mol.nao, int(mf.grids.size)
    gga = mf.xctype == "GGA"
    nk = 4 if gga else 1
    st = {}
    rng = np.random.default_rng(0)
    x_s = rng.standard_normal((n, n)) * 0.05
    x_s = x_s + x_s.T
    kern = torch.as_tensor(mcol.sf_mc_kernel(td.mf, gm.collinear_samples, device=0), device=eng.dev)
    eng.fxc_sf_response(x_s, kern, want=("v", "wv"), stats=st)
    m = min(ng, st["chunk"])
    res["fxc_sf_response"] = dict(gemm_s=st["gemm_s"], xc_resp_sf_s=st["xc_resp_sf_s"], chunk=st["chunk"], chunks=st["chunks"])
    ao, w = eng.ao, eng.w
    aoc = ao[:, :m].contiguous()
    c = (aoc[0] @ torch.as_tensor(x_s, device=eng.dev)).contiguous()
    f_c, w_c = kern[..., :m].contiguous(), w[:m].contiguous()
    rho1 = torch.zeros((4, m), dtype=torch.float64, device=eng.dev)
    wv = torch.zeros_like(rho1)
    b = torch.empty((m, n), dtype=torch.float64, device=eng.dev)
    wv2 = torch.as_tensor(rng.standard_normal((2, 4, m)), device=eng.dev) * w_c
    b2 = torch.empty((2, m, n), dtype=torch.float64, device=eng.dev)
    L = _capi.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(eng.dev).cuda_stream)

    def k_resp():
        _capi.check(L.xt_xc_resp_sf(m, n, _capi.XC[mf.xctype], aoc.data_ptr(), aoc.stride(0), n, c.data_ptr(), n,
                                    f_c.data_ptr(), m, w_c.data_ptr(), rho1.data_ptr(), wv.data_ptr(), m, b.data_ptr(), n,
                                    stream), "xt_xc_resp_sf")

    def k_rows():
        _capi.check(L.xt_xc_rows(m, n, _capi.XC[mf.xctype], 2, aoc.data_ptr(), aoc.stride(0), n, wv2.data_ptr(), m,
                                 b2.data_ptr(), n, stream), "xt_xc_rows")

    def timed(f):
        f()
        ts = []
        for _ in range(a.reps):
            t0 = sync()
            f()
            ts.append(sync() - t0)
        return float(np.median(ts)), float(min(ts))
    plane = 8 * m * n
    kr, kr_min = timed(k_resp)
    tr, tr_min = timed(lambda: torch_resp_sf(torch, aoc, c, f_c, w_c, gga))
    ko, ko_min = timed(k_rows)
    to, to_min = timed(lambda: torch_rows(torch, aoc, wv2, gga))
    t_rho, t_wv, t_b = torch_resp_sf(torch, aoc, c, f_c, w_c, gga)
    t_b2 = torch_rows(torch, aoc, wv2, gga)
    kr_bytes = plane * (2 * nk + 2) + 8 * m * (nk * nk + 1 + 2 * nk)          # ao twice (two passes), c and b once
    tr_bytes = plane * (3 * nk + (2 * nk + 2))           # (read 2, write 1) per component; b: read, write, reduce
    ko_bytes = plane * (nk + 2) + 8 * m * 2 * nk                                # ao once for both channels, b twice
    to_bytes = 2 * plane * (2 * nk + 2)
    res["xt_xc_resp_sf_vs_torch"] = dict(
        points=m, nao=n, xctype=mf.xctype, kernel_s_median=kr, kernel_s_min=kr_min, torch_s_median=tr, torch_s_min=tr_min,
        kernel_bytes=kr_bytes, torch_bytes=tr_bytes, kernel_gb_per_s=kr_bytes / kr * 1e-9, torch_gb_per_s=tr_bytes / tr * 1e-9,
        speedup=tr / kr, max_abs_diff=dict(rho1=float((rho1[:nk] - t_rho).abs().max()), wv=float((wv[:nk] - t_wv).abs().max()),
                                           b=float((b - t_b).abs().max())))
    res["xt_xc_rows_vs_torch"] = dict(
        points=m, nao=n, channels=2, kernel_s_median=ko, kernel_s_min=ko_min, torch_s_median=to, torch_s_min=to_min,
        kernel_bytes=ko_bytes, torch_bytes=to_bytes, kernel_gb_per_s=ko_bytes / ko * 1e-9, torch_gb_per_s=to_bytes / to * 1e-9,
        speedup=to / ko, max_abs_diff=float((b2 - t_b2).abs().max()))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
