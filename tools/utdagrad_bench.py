"""Device timing of the U-TDA gradient on a UKS reference (``xtddft_amd.grad_utda.UTDAGradients``;
kernels ``xt_grad_jk2``, ``xt_grad_xc``, ``xt_xc_resp`` and ``xt_xc_rows``) on one molecule of a real
size: naphthalene+ / cc-pVDZ, UKS / B3LYP, state 1, the molecule of ``tools/sfksgrad_bench.py``.

    python tools/utdagrad_bench.py [--molecule naphthalene+] [--xc b3lyp] [--out profiles/utdagrad_bench.json]

Recorded, from the second of two gradient evaluations: the timing keys of ``tools/sfksgrad_bench.py``
(host one-electron part, the two-electron launches, the Z-vector solve, ``fxc_response``, the G_xc
pairs) and the seconds of the third-derivative weights.  In the same run, on the pair lists of that
state (``grad_utda.jk_lists`` at D = D0 + T, without the Z-vector's part, which changes no cost): one
``xt_grad_jk2`` call against the same pairs sent as two ``xt_grad_jk`` calls, ms of the launches and
the largest difference of the two results; and ``qc.xc.kernel_grad_torch`` on the grid of the mean
field.  Recorded, not gated: the driver uses whichever route this file shows faster.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def two_call_terms(jl, kl, max_terms):
    """The pairs of ``grad_utda.jk_lists`` as the terms of ``xt_grad_jk`` calls of at most ``max_terms`` pairs
    each (every pair with one zero weight): what a gradient without ``xt_grad_jk2`` would have to send."""
    terms = [(w, 0.0, p, q) for w, p, q in jl] + [(0.0, w, p, q) for w, p, q in kl]
    return [terms[i:i + max_terms] for i in range(0, len(terms), max_terms)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--xc", default="b3lyp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "utdagrad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import build, grad_utda
    from xtddft_amd.qc import M, UKS
    from xtddft_amd.qc import grad as G
    from xtddft_amd.qc import xc as _xc
    from xtddft_amd.xtda import XTDA
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("utdagrad_bench needs the GPU: nothing is measured without one")
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
    td = XTDA(mol, mf.to_meanfield(), nstates=2, use_Davidson=True)
    td.conv_tol = 1e-6
    td.kernel()
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
        kernel_grad_s=tm["kernel_grad_s"], xc_rows_s=tm["xc_rows_s"],
        grad_xc_pairs_s=tm["grad_xc_s"], grad_xc_gemm_s=sx["gemm_s"], grad_xc_kernel_s=sx["grad_xc_s"],
        grad_xc_bytes=sx["grad_xc_bytes"], max_abs_g=float(np.abs(de).max()), max_abs_g_xc=float(np.abs(gm.de_xc).max()),
        sum_g=[float(x) for x in de.sum(axis=0)])

    # one xt_grad_jk2 call against the same pairs as two xt_grad_jk calls
    scf = gm._scf
    x = grad_utda.utda_amplitudes(td, 0)
    C = [np.asarray(scf.mo_coeff[s]) for s in range(2)]
    occ = [np.asarray(scf.mo_occ[s]) > 0 for s in range(2)]
    o = [C[s][:, occ[s]] for s in range(2)]
    v = [C[s][:, ~occ[s]] for s in range(2)]
    d0 = np.asarray([o[s] @ o[s].T for s in range(2)])
    t = np.asarray([v[s] @ x[s] @ x[s].T @ v[s].T - o[s] @ x[s].T @ x[s] @ o[s].T for s in range(2)])
    xt = np.asarray([v[s] @ x[s] @ o[s].T for s in range(2)])
    jl, kl = grad_utda.jk_lists(d0 + t, t, xt, float(scf.hyb))
    dev = scf._device
    s1, s2 = {}, {}
    t0 = sync()
    one = G.grad_jk_lists(mol, jl, kl, dev, stats=s1)
    one_call_s = sync() - t0
    t0 = sync()
    calls = two_call_terms(jl, kl, G.MAX_TERMS)
    two = sum(G.grad_jk_device(mol, terms, dev, stats=s2) for terms in calls)
    two_call_s = sync() - t0
    res["one_call_vs_two_calls"] = dict(
        coulomb_pairs=len(jl), exchange_pairs=len(kl),
        xt_grad_jk2_ms=sum(b["ms"] for b in s1["buckets"]), xt_grad_jk2_call_s=one_call_s,
        two_xt_grad_jk_ms=sum(b["ms"] for b in s2["buckets"]), two_xt_grad_jk_call_s=two_call_s,
        calls_of_xt_grad_jk=len(calls), max_abs_diff=float(np.abs(one - two).max()),
        max_abs=float(np.abs(one).max()), faster="xt_grad_jk2" if one_call_s < two_call_s else "two xt_grad_jk calls")

    # the third-derivative weights on the grid of the mean field
    eng = mf.device_engine
    nk = 4 if eng.xctype == "GGA" else 1
    xs = (xt + xt.transpose(0, 2, 1)) * 0.5
    rho1 = eng.fxc_response(xs, want=("rho1",))["rho1"][:, :nk]
    with torch.cuda.device(eng.dev):
        rho0 = eng.rho(d0)[:, :nk]
        ts = []
        for _ in range(3):
            t0 = sync()
            q, dq = _xc.kernel_grad_torch(mf.xc, rho0, rho1)
            ts.append(sync() - t0)
    res["kernel_grad_torch"] = dict(points=int(rho0.shape[-1]), seconds_min=float(min(ts)), seconds_first=float(ts[0]),
                                    omega_xc=float((q * eng.w).sum()), max_abs_dq=float(dq.abs().max()))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
