"""Generator of tests/golden/grad_kappa.json: run by hand on a CPU with mpmath installed,

    python tests/golden/make_grad_kappa.py

For every case of tests/grad_cases.py it compares the host FP64 restatement of the call
(hint_ref.host_grad: float64 integrals by the formula of ints.eri_quartet, times Gamma, summed in
float64) with the 40-digit reference (hint_ref.ref_grad) and records, per total order L, the
host's largest error in units of 2^-53 sabs (`host_error`) and kappa_g(L) = max(64, 8 x that)
(`kappa_g`).  A figure above kappa(L) + n (kappa(L) of tests/golden/int_ref.npz, n the number of
products summed into the entry: Higham's gamma_n on top of the integrals' own bound) would mean
that the host restatement is wrong; the script refuses to write it.  The file holds numbers only.
It prints the table; DESIGN.md records it.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import grad_cases as gc     # noqa: E402
import hint_ref             # noqa: E402
import int_cases as ic      # noqa: E402


def main():
    kappa = ic.load_fixture()["kappa"]
    measured = np.zeros(gc.L_MAX + 1)
    for c in gc.REF_CASES:
        call = gc.build(c)
        ref, sabs, Lrow, nsum = hint_ref.ref_grad(call)
        host = hint_ref.host_grad(call)
        un = gc.units(host, ref, sabs, Lrow).max(axis=1)
        for A in np.flatnonzero(Lrow >= 0):
            assert gc.KAPPA_FACTOR * un[A] <= kappa[Lrow[A]] + nsum[A], (c.name, A, un[A], nsum[A])
        measured = np.maximum(measured, gc.measured_ratio(host, ref, sabs, Lrow))
        print(f"{c.name:12s} L {int(Lrow.max()):2d}  host {un.max():8.2f} units", flush=True)
    kg = gc.kappa_from(measured)
    with open(gc.kappa_file(), "w") as f:
        json.dump(dict(host_error=[round(float(x), 4) for x in measured], kappa_g=[round(float(x), 4) for x in kg]), f)
        f.write("\n")
    print("\n L   host error / (2^-53 sabs)   kappa_g(L)")
    for L in range(1, gc.L_MAX + 1):
        print(f"{L:2d}   {measured[L]:12.2f}              {kg[L]:10.1f}")


if __name__ == "__main__":
    main()
