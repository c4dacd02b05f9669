"""Device timing of the UKS ground-state gradient (``qc.grad.KSGradients``; kernels ``xt_grad_jk``
and ``xt_grad_xc``) on one molecule of a real size: naphthalene+ / cc-pVDZ, UKS / B3LYP, the
molecule of ``tools/grad_bench.py``.

    python tools/ksgrad_bench.py [--molecule naphthalene+] [--xc b3lyp] [--out profiles/ksgrad_bench.json]

Recorded, from the second of two gradient evaluations (the first one fills the Boys table and the
table caches): seconds of the host one-electron part, of ``xt_grad_jk`` (the launches, and the
call with its table set-up), of the GEMMs that form e and c on the engine, and of ``xt_grad_xc``
(host clock around work that ends in a device synchronise), and the rate at which ``xt_grad_xc``
read its operands: the bytes of e, c and the three gradient planes of h per spin over its time.
The yardstick for that rate is the read stream of ``tools/stream_probe.py``.
Every block of a grid tile re-reads h and the coordinates from cache; those re-reads are not
counted.  Recorded, not gated.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--xc", default="b3lyp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksgrad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import build
    from xtddft_amd.qc import M, UKS
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("ksgrad_bench needs the GPU: nothing is measured without one")
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
    gm = mf.nuc_grad_method()
    runs = []
    for _ in range(2):
        t0 = sync()
        de = gm.kernel()
        runs.append((sync() - t0, dict(gm.timings)))
    total_s, tm = runs[1]
    res["gradient"] = dict(
        total_s=total_s, warmup_total_s=runs[0][0], one_electron_s=tm["one_electron_s"],
        grad_jk_s=sum(b["ms"] for b in tm["buckets"]) * 1e-3, grad_jk_call_s=tm["grad_jk_s"],
        gemm_s=tm["gemm_s"], grad_xc_s=tm["grad_xc_s"], grad_xc_call_s=tm["grad_xc_call_s"],
        grad_xc_bytes=tm["grad_xc_bytes"], grad_xc_read_gb_per_s=tm["grad_xc_bytes"] / tm["grad_xc_s"] * 1e-9,
        chunk=tm["chunk"], chunks=tm["chunks"], max_abs_g=float(np.abs(de).max()),
        max_abs_g_xc=float(np.abs(gm.de_xc).max()), sum_g=[float(x) for x in de.sum(axis=0)])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
