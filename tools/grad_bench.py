"""Device timing of the analytic spin-flip CIS gradient (``xtddft_amd.grad``; kernel ``xt_grad_jk``)
on one molecule of a real size: naphthalene+ / cc-pVDZ UHF, the molecule of ``tools/somf_bench.py``.

    python tools/grad_bench.py [--molecule naphthalene+] [--state 1] [--out profiles/grad_bench.json]

Recorded: quartets (bra entries x ket entries), the flop estimate and wall ms of ``xt_grad_jk`` per
(bra bucket, ket bucket) launch (host clock around a launch that ends in a device synchronise, the
second of two gradient evaluations: the first one fills the Boys table and the table caches),
Z-vector iterations and time, the host one-electron time and the total.  For scale, the time of
one SCF + SF-TDA energy evaluation in the same run: a central finite-difference gradient costs
6 natm of those, and it is the only baseline the code before this tool offers.  Recorded, not gated.

The flop estimate counts, per primitive quartet of order L = l_bra + l_ket, the R_tuv recursion
(3 flops per entry of every level), the ket contraction M (2 ntuv(l_bra) ntuv(l_ket) per ket
component) and the three bra contractions (6 ntuv(l_bra) per integral position); Gamma and the
Boys function are left out.  HBM traffic is the tables, the densities and the partial sums
(bytes_min): the kernel is bound by its arithmetic and its private arrays, not by HBM.
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


def ntuv(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


def flop_estimate(tab, b0, b1, k0, k1):
    """Floating-point operations of one launch over bra entries [b0, b1) and ket entries [k0, k1)."""
    bi, ki = tab.bra.info[b0:b1].astype(np.int64), tab.ket_info[k0:k1].astype(np.int64)
    lb, nab, npp = bi[:, 0][:, None], (bi[:, 1] // 3)[:, None], bi[:, 2][:, None]
    lk, nr, ncd = ki[:, 0][None, :], ki[:, 1][None, :], ki[:, 5][None, :]
    L = lb + lk
    rec = np.zeros_like(L)
    for m in range(1, 15):
        rec += np.where(L >= m, 3 * ntuv(m), 0)
    ntb, ntk = ntuv(lb), ntuv(lk)
    per_prim = rec + ncd * (2 * ntb * ntk + nab * 6 * ntb)
    return float((npp * nr * per_prim).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--state", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_bench.json"))
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import build
    from xtddft_amd.qc import M, UHF
    from xtddft_amd.qc import grad as G
    from xtddft_amd.sf_tda import SF_TDA_down
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("grad_bench needs the GPU: nothing is measured without one")
    spec = MOLECULES[a.molecule]
    mol = M(spec["atom"], basis=spec["basis"], charge=spec.get("charge", 0), spin=spec.get("spin", 0),
            unit=spec.get("unit", "Angstrom"))

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def energy():
        t0 = sync()
        mf = UHF(mol)
        mf.conv_tol = 1e-10
        mf.max_cycle = 200
        mf.to_device(0).cholesky(1e-12)
        mf.kernel()
        t1 = sync()
        td = SF_TDA_down(mf.to_meanfield(), method=0, davidson=True)
        td.kernel(nstates=max(3, a.state))
        t2 = sync()
        return mf, td, t1 - t0, t2 - t1
    energy()                                             # warm-up: code objects, Cholesky plan
    mf, td, scf_s, tda_s = energy()
    res = dict(molecule=spec.get("label", a.molecule), nao=mol.nao, natm=mol.natm, nshell=len(mol.shells),
               device=torch.cuda.get_device_name(0), scf_converged=bool(mf.converged), e_tot=float(mf.e_tot),
               state=a.state, omega_ha=float(td.e[a.state - 1]),
               energy_eval=dict(scf_s=scf_s, sf_tda_s=tda_s, total_s=scf_s + tda_s,
                                finite_difference_gradient_s=6 * mol.natm * (scf_s + tda_s)))
    t0 = time.perf_counter()
    tab = G.grad_tables(mol)
    tab.dev(0), tab.bra.dev(0), tab.ket.dev(0)
    res["table_build_s"] = time.perf_counter() - t0
    gm = td.nuc_grad_method()
    runs = []
    for _ in range(2):
        t0 = sync()
        de = gm.kernel(state=a.state)
        runs.append((sync() - t0, dict(gm.timings)))
    total_s, tm = runs[1]
    ranges = [(b, k) for b in tab.bra_ranges for k in tab.ket_ranges]
    buckets = []
    for row, ((b0, b1, _), (k0, k1, _)) in zip(tm["buckets"], ranges):
        fl = flop_estimate(tab, b0, b1, k0, k1)
        buckets.append(dict(row, flops_est=fl, gflops_est=fl / (row["ms"] * 1e-3) * 1e-9))
    bytes_min = 8.0 * (tab.bra.eb.size + tab.bra.prim.size + tab.ket.eab.size + tab.ket.pprim.size
                       + 2 * 8 * tab.ncart ** 2) + 4.0 * (tab.bra.info.size + tab.ket_info.size)
    res["gradient"] = dict(total_s=total_s, warmup_total_s=runs[0][0], grad_jk_ms=sum(b["ms"] for b in buckets),
                           grad_jk_call_s=tm["grad_jk_s"], buckets=buckets,
                           flops_est=sum(b["flops_est"] for b in buckets), bytes_min=bytes_min,
                           zvector_cycles=tm["zvector_cycles"], zvector_s=tm["zvector_s"],
                           zvector_residual=tm["zvector_residual"], one_electron_s=tm["one_electron_s"],
                           max_abs_g=float(np.abs(de).max()), sum_g=[float(x) for x in de.sum(axis=0)])
    res["gradient"]["vs_finite_difference"] = res["energy_eval"]["finite_difference_gradient_s"] / total_s
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
