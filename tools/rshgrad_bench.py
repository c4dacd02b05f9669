"""Device timing of the range-separated gradients (``xt_grad_jk2_lr`` next to ``xt_grad_jk2``;
``qc.grad.grad_jk_rsh``) on one molecule of a real size: naphthalene+ / cc-pVDZ, UKS / CAM-B3LYP, the
molecule of ``tools/utdagrad_bench.py``.

    python tools/rshgrad_bench.py [--molecule naphthalene+] [--xc cam-b3lyp] [--out profiles/rshgrad_bench.json]

Two gradients through ``.Gradients()``: the ground state and U-TDA state 1.  For each, from three repeats
after one warm-up evaluation: the wall time of the long-range call (``xt_grad_jk2_lr``: the exchange pairs
only, weighted by alpha - hyb) and of the full-range call of the same gradient (``xt_grad_jk2``: the Coulomb
list and the same exchange pairs weighted by hyb), both over the same quartets -- the sum of the launches'
synchronised wall ms -- with the spread of the repeats, and the other timing keys of the driver.  The
expectation "about the time of the full-range call, and no more than it" is read off these two numbers;
nothing is gated here.
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

REPEATS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--xc", default="cam-b3lyp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rshgrad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import build
    from xtddft_amd.qc import M, UKS
    from xtddft_amd.xtda import XTDA
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("rshgrad_bench needs the GPU: nothing is measured without one")
    spec = MOLECULES[a.molecule]
    mol = M(spec["atom"], basis=spec["basis"], charge=spec.get("charge", 0), spin=spec.get("spin", 0),
            unit=spec.get("unit", "Angstrom"))

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    t0 = sync()
    mf = UKS(mol, xc=a.xc)
    # converged as the gradient tests converge it: the drivers check the omega of their own coupling (full
    # F_oo / F_vv blocks) against the TDA root (orbital-energy differences) to 1e-9 Ha, and an SCF stopped at
    # 1e-10 in the energy leaves off-diagonal Fock elements that show there (6e-8 Ha on this molecule)
    mf.conv_tol = 1e-12
    mf.conv_tol_grad = 1e-9
    mf.max_cycle = 300
    mf.to_device(0).cholesky(1e-12)
    mf.kernel()
    scf_s = sync() - t0
    if not mf.omega > 0:
        raise SystemExit(f"{a.xc} is not range-separated: there is no long-range call to time")
    res = dict(molecule=spec.get("label", a.molecule), xc=a.xc, omega=float(mf.omega), hyb=float(mf.hyb),
               alpha=float(mf.alpha), nao=mol.nao, natm=mol.natm, nshell=len(mol.shells), ngrid=int(mf.grids.size),
               device=torch.cuda.get_device_name(0), scf_converged=bool(mf.converged), e_tot=float(mf.e_tot),
               scf_s=scf_s, repeats=REPEATS)

    def timed(gm, **kw):
        """One warm-up, then REPEATS evaluations: the two calls' launch ms per repeat, and the last timings."""
        gm.kernel(**kw)
        full, lr, total = [], [], []
        for _ in range(REPEATS):
            t0 = sync()
            de = gm.kernel(**kw)
            total.append(sync() - t0)
            tm = dict(gm.timings)
            full.append(sum(b["ms"] for b in tm["buckets"]))
            lr.append(sum(b["ms"] for b in tm["buckets_lr"]))
        pairs = dict(quartets=int(sum(b["quartets"] for b in tm["buckets"])), launches=len(tm["buckets"]),
                     launches_lr=len(tm["buckets_lr"]))
        out = dict(total_s=float(min(total)), xt_grad_jk2_ms=[float(x) for x in full],
                   xt_grad_jk2_lr_ms=[float(x) for x in lr], xt_grad_jk2_ms_min=float(min(full)),
                   xt_grad_jk2_lr_ms_min=float(min(lr)), xt_grad_jk2_spread_ms=float(max(full) - min(full)),
                   xt_grad_jk2_lr_spread_ms=float(max(lr) - min(lr)), lr_over_full=float(min(lr) / min(full)),
                   buckets=tm["buckets"], buckets_lr=tm["buckets_lr"], one_electron_s=tm["one_electron_s"],
                   max_abs_g=float(np.abs(de).max()), sum_g=[float(x) for x in de.sum(axis=0)], **pairs)
        for key in ("zvector_s", "zvector_cycles", "zvector_residual", "xc_response_s", "xc_response_calls",
                    "kernel_grad_s", "grad_xc_s"):
            if key in tm:
                out[key] = tm[key]
        return out

    res["ground_state"] = dict(coulomb_pairs=1, exchange_pairs=2, **timed(mf.Gradients()))
    t0 = sync()
    td = XTDA(mol, mf.to_meanfield(), nstates=2, use_Davidson=True)
    td.conv_tol, td.lindep = 1e-8, 1e-20     # residual norm below 1e-8; no correction vector dropped above it
    td.kernel()
    res["tda"] = dict(seconds=sync() - t0, omega=[float(x) for x in np.asarray(td.e)[:2]],
                      converged=[bool(x) for x in np.asarray(td.converged)[:2]])
    res["utda_state_1"] = dict(coulomb_pairs=3, exchange_pairs=8, **timed(td.Gradients(state=1)))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
