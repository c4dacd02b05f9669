"""Device timing of the collinear spin-flip TDA gradient on a UKS reference
(``xtddft_amd.grad.SFGradients``; kernels ``xt_grad_jk``, ``xt_grad_xc`` and ``xt_xc_resp``) on one
molecule of a real size: naphthalene+ / cc-pVDZ, UKS / B3LYP, spin-flip-down state 1, the molecule of
``tools/grad_bench.py`` and ``tools/ksgrad_bench.py``.

    python tools/sfksgrad_bench.py [--molecule naphthalene+] [--xc b3lyp] [--out profiles/sfksgrad_bench.json]

Recorded, from the second of two gradient evaluations: the seconds of the host one-electron part, of
``xt_grad_jk``, of the Z-vector solve (total and per cycle), of ``fxc_response`` per call (its GEMMs
and ``xt_xc_resp`` apart) and of the two G_xc pairs.  On the same data (c = phi dm of a random
symmetric density pair, the engine's AO planes, fxc and weights) ``xt_xc_resp`` is timed against the
same rho1, wv and b composed from torch operations the way ``DeviceEngine.vxc`` composes its
potential, with the bytes each side moves: the kernel's operands and results once each; for torch
every G x nao plane an operation reads or writes (counted from the operations, not from hardware
counters).  The yardsticks are the streams of ``tools/stream_probe.py``.
Recorded, not gated.
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


def torch_response(torch, ao, c, fxc, w, gga):
    """rho1, wv (unhalved) and b from torch passes over the G x nao planes."""
    nc = 4 if gga else 1
    rho = [torch.stack([(ao[0] * c[s]).sum(1)] + [2.0 * (ao[k] * c[s]).sum(1) for k in range(1, nc)]) for s in range(2)]
    rho1 = torch.stack(rho)
    wv = torch.einsum('skrlg,rlg->skg', fxc, rho1) * w
    b = []
    for s in range(2):
        h = wv[s].clone()
        if gga:
            h[0] *= 0.5
        b.append((h[:nc, :, None] * ao[:nc]).sum(0))
    return rho1, wv, torch.stack(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--xc", default="b3lyp")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfksgrad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import _capi, build
    from xtddft_amd.qc import M, UKS
    from xtddft_amd.sf_tda import SF_TDA_down
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("sfksgrad_bench needs the GPU: nothing is measured without one")
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
    td = SF_TDA_down(mf.to_meanfield(), method=2, davidson=True, conv_tol=1e-10, tol_residual=1e-6)
    td.kernel(nstates=2)
    res["tda"] = dict(seconds=sync() - t0, omega=[float(x) for x in np.asarray(td.e)[:2]],
                      converged=[bool(x) for x in np.asarray(td.converged)[:2]])
    gm = td.nuc_grad_method()
    runs = []
    for _ in range(2):
        t0 = sync()
        de = gm.kernel(state=1)
        runs.append((sync() - t0, dict(gm.timings)))
    total_s, tm = runs[1]
    sx = tm["grad_xc_stats"]
    res["gradient"] = dict(
        total_s=total_s, warmup_total_s=runs[0][0], one_electron_s=tm["one_electron_s"],
        grad_jk_s=sum(b["ms"] for b in tm["buckets"]) * 1e-3, grad_jk_call_s=tm["grad_jk_s"],
        zvector_s=tm["zvector_s"], zvector_cycles=tm["zvector_cycles"], zvector_residual=tm["zvector_residual"],
        zvector_s_per_cycle=tm["zvector_s"] / max(1, tm["zvector_cycles"]),
        xc_response_s=tm["xc_response_s"], xc_response_calls=tm["xc_response_calls"],
        grad_xc_pairs_s=tm["grad_xc_s"], grad_xc_gemm_s=sx["gemm_s"], grad_xc_kernel_s=sx["grad_xc_s"],
        grad_xc_bytes=sx["grad_xc_bytes"], max_abs_g=float(np.abs(de).max()), max_abs_g_xc=float(np.abs(gm.de_xc).max()),
        sum_g=[float(x) for x in de.sum(axis=0)])

    # fxc_response per call, its parts apart
    eng = mf.device_engine
    n, ng = mol.nao, int(mf.grids.size)
    rng = np.random.default_rng(0)
    dm = rng.standard_normal((2, n, n)) * 0.05
    dm = dm + dm.transpose(0, 2, 1)
    eng.fxc_response(dm, want=("v",))
    calls = []
    for _ in range(5):
        st = {}
        t0 = sync()
        eng.fxc_response(dm, want=("v",), stats=st)
        st["call_s"] = sync() - t0
        calls.append(st)
    best = min(calls, key=lambda s: s["call_s"])
    res["fxc_response"] = dict(call_s=best["call_s"], gemm_s=best["gemm_s"], xc_resp_s=best["xc_resp_s"],
                               xc_resp_bytes=best["xc_resp_bytes"], chunk=best["chunk"], chunks=best["chunks"])

    # xt_xc_resp against the torch composition on the same data (one chunk of the grid)
    gga = mf.xctype == "GGA"
    nc = 4 if gga else 1
    m = min(ng, best["chunk"])
    ao, fxc, w = eng.ao, eng.fxc_ground(), eng.w
    dmt = torch.as_tensor(dm, device=eng.dev)
    c = torch.stack([ao[0, :m] @ dmt[s] for s in range(2)]).contiguous()
    aoc = ao[:, :m].contiguous()
    fxc_c, w_c = fxc[..., :m].contiguous(), w[:m].contiguous()
    rho1 = torch.zeros((2, 4, m), dtype=torch.float64, device=eng.dev)
    wv = torch.zeros_like(rho1)
    b = torch.empty((2, m, n), dtype=torch.float64, device=eng.dev)
    L = _capi.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(eng.dev).cuda_stream)

    def kernel():
        _capi.check(L.xt_xc_resp(m, n, _capi.XC[mf.xctype], aoc.data_ptr(), aoc.stride(0), n, c.data_ptr(), n,
                                 fxc_c.data_ptr(), m, w_c.data_ptr(), rho1.data_ptr(), wv.data_ptr(), m, b.data_ptr(), n,
                                 stream), "xt_xc_resp")

    def timed(f):
        f()
        ts = []
        for _ in range(a.reps):
            t0 = sync()
            f()
            ts.append(sync() - t0)
        return float(np.median(ts)), float(min(ts))
    k_med, k_min = timed(kernel)
    t_med, t_min = timed(lambda: torch_response(torch, aoc, c, fxc_c, w_c, gga))
    tr, tw, tb = torch_response(torch, aoc, c, fxc_c, w_c, gga)
    plane = 8 * m * n
    k_bytes = plane * ((nc + 2) + (nc + 2)) + 8 * m * (4 * nc * nc + 1 + 4 * nc)     # ao twice (two passes), c and b once
    t_bytes = 2 * plane * (4 * nc + (2 * nc + nc + 1))       # per spin: (read 2, write 1, read 1) per component; b: read, write, reduce
    res["xt_xc_resp_vs_torch"] = dict(
        points=m, nao=n, xctype=mf.xctype, kernel_s_median=k_med, kernel_s_min=k_min, torch_s_median=t_med,
        torch_s_min=t_min, kernel_bytes=k_bytes, torch_bytes=t_bytes, kernel_gb_per_s=k_bytes / k_med * 1e-9,
        torch_gb_per_s=t_bytes / t_med * 1e-9, speedup=t_med / k_med,
        max_abs_diff=dict(rho1=float((rho1[:, :nc] - tr).abs().max()), wv=float((wv[:, :nc] - tw).abs().max()),
                          b=float((b - tb).abs().max())))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
