"""Device timing of the spin-orbit mean-field contraction (``qc.dints.somf_g_device``: kernel
``xt_hint_cart`` in cross mode, the spherical transforms and the digestion) on one molecule of
a real size, with the one-centre approximation on and off, next to ``eri_full_device`` on the
same molecule in the same run.

    python tools/somf_bench.py [--molecule naphthalene+] [--chunk-pairs N] [--out profiles/somf_bench.json]

The table build is host time (perf_counter); kernel, transforms and contractions are HIP events
around every launch / block of the chunk loop, summed after the final synchronise; ``total`` is
one pair of events around the whole call, its synchronise included.  There is no earlier device
time and no reference time for this path.  The yardstick is the plain ERI kernel: seconds per
Cartesian integral component of ``xt_hint_cart`` (3 components per (ab|cd) position of the
ordered pair tables) over seconds per component of ``xt_int2e_cart`` (one launch of
``eri_full_device``'s i >= j pair table against itself).  Recorded, not gated.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecule", default="naphthalene+")
    ap.add_argument("--chunk-pairs", type=int, default=None)
    ap.add_argument("--skip-full", action="store_true", help="one-centre run only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from molecule_run import MOLECULES
    from xtddft_amd import _capi, build
    from xtddft_amd.qc import M, dints
    build.build()
    L = _capi.lib()
    spec = MOLECULES[a.molecule]
    mol = M(spec["atom"], basis=spec["basis"], charge=spec.get("charge", 0), spin=spec.get("spin", 0))
    n = mol.nao
    rng = np.random.default_rng(0)
    x, y, z = (rng.standard_normal((n, n)) for _ in range(3))
    dens = dict(pLL=x + x.T, pLS=y, pSS=z + z.T)

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # the yardstick: one xt_int2e_cart launch of the i >= j pair table against itself
    tab = dints.pair_table(mol)
    d = tab.dev(0)
    kinfo = torch.as_tensor(tab.ket_info_pairs(np.arange(tab.npair), tab.c0.astype(np.int32)), device="cuda")
    cart = torch.zeros((tab.ncart_tot, tab.ncart_tot), dtype=torch.float64, device="cuda")
    eri_s = []
    for _ in range(2):                                   # the first launch fills the Boys table
        cart.zero_()
        e0, e1 = events()
        e0.record()
        dints._launch(L, tab, d, tab.npair, kinfo, d["pprim"], d["eab"], 2 * tab.lmax, 0.0, cart, tab.ncart_tot, 0)
        e1.record()
        torch.cuda.synchronize()
        eri_s.append(e0.elapsed_time(e1) * 1e-3)
    del cart
    eri_comp = float(tab.ncart_tot) ** 2
    res = dict(molecule=spec.get("label", a.molecule), nao=n, nshell=len(mol.shells), device=torch.cuda.get_device_name(0),
               eri=dict(pairs=tab.npair, components=eri_comp, kernel_s=eri_s[1], first_launch_s=eri_s[0],
                        s_per_component=eri_s[1] / eri_comp))
    print(json.dumps(res["eri"]))
    for use_1c in ([True] if a.skip_full else [True, False]):
        t0 = time.perf_counter()
        dt = dints.deriv_pair_table(mol, use_1c)
        dt.dev(0)
        build_s = time.perf_counter() - t0
        if use_1c:
            comp = 3.0 * sum(float(dt.nab[dt.atom == at].sum()) ** 2 for at in set(dt.atom.tolist()))
        else:
            comp = 3.0 * float(dt.ncart_tot) ** 2
        runs = []
        for _ in range(2):                               # warm-up, then the recorded run
            tm = {}
            e0, e1 = events()
            e0.record()
            g = dints.somf_g_device(mol, **dens, use_1c=use_1c, chunk_pairs=a.chunk_pairs, timings=tm)
            e1.record()
            torch.cuda.synchronize()
            tm["total"] = e0.elapsed_time(e1) * 1e-3
            runs.append(tm)
        tm = runs[1]
        row = dict(use_1c=use_1c, pairs=dt.npair, chunk_pairs=dints.somf_chunk_pairs(dt, 0, a.chunk_pairs),
                   components=comp, table_build_s=build_s, kernel_s=tm["kernel"], transform_s=tm["transform"],
                   contract_s=tm["contract"], total_s=tm["total"], warmup_total_s=runs[0]["total"],
                   s_per_component=tm["kernel"] / comp,
                   per_component_vs_eri=(tm["kernel"] / comp) / res["eri"]["s_per_component"],
                   max_abs_g=[float(np.abs(v).max()) for v in g])
        print(json.dumps(row))
        res["1c" if use_1c else "full"] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
