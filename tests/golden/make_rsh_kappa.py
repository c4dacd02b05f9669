"""Generator of tests/golden/rsh_kappa.json: run by hand on a CPU with mpmath installed,

    python tests/golden/make_rsh_kappa.py

The rule of make_grad_kappa.py for the long-range entry ``xt_grad_jk2_lr``: for every raw call of
``rsh_ref.bound_cases()`` (the 49 classes, the structure cases and the far pair at omega = 0.33, one case
per template instance at omega = 0.2, 2^-4 and 16) it compares the host FP64 restatement
(``rsh_ref.host_grad_lr``: ``hint_ref.host_integrals`` with ``ints._attenuate``) with the 40-digit reference
(``rsh_ref.grad_integrals_lr`` through ``hint_ref.ref_grad``) and records, per total order L, the host's
largest error in units of 2^-53 sabs (`host_error`) and kappa_lr(L) = max(64, 8 x that) (`kappa_lr`).  The
sanity bound of make_grad_kappa.py (kappa(L) of the integral fixture + the number of products summed)
applies unchanged.  The file holds numbers only.  It prints the table; DESIGN.md section 20 records it.
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
import rsh_ref              # noqa: E402


def main():
    kappa = ic.load_fixture()["kappa"]
    measured = np.zeros(gc.L_MAX + 1)
    for name, c, call, omega in rsh_ref.bound_cases():
        ref, sabs, Lrow, nsum = hint_ref.ref_grad(call, blocks=rsh_ref.grad_integrals_lr(call, omega))
        host = rsh_ref.host_grad_lr(call, omega)
        un = gc.units(host, ref, sabs, Lrow).max(axis=1)
        for A in np.flatnonzero(Lrow >= 0):
            assert gc.KAPPA_FACTOR * un[A] <= kappa[Lrow[A]] + nsum[A], (name, A, un[A], nsum[A])
        measured = np.maximum(measured, gc.measured_ratio(host, ref, sabs, Lrow))
        print(f"{name:14s} omega {omega:<7g} L {int(Lrow.max()):2d}  host {un.max():8.2f} units", flush=True)
    kl = gc.kappa_from(measured)
    with open(rsh_ref.kappa_file(), "w") as f:
        json.dump(dict(host_error=[round(float(x), 4) for x in measured], kappa_lr=[round(float(x), 4) for x in kl]), f)
        f.write("\n")
    print("\n L   host error / (2^-53 sabs)   kappa_lr(L)")
    for L in range(1, gc.L_MAX + 1):
        print(f"{L:2d}   {measured[L]:12.2f}              {kl[L]:10.1f}")


if __name__ == "__main__":
    main()
