"""Generator of tests/golden/int_ref.npz: run by hand on a CPU with mpmath installed,

    python tests/golden/make_int_ref.py

For every case of tests/int_cases.py that owns a fixture entry it stores, under the case's
name, `<name>/ref` (the 40-digit reference of tests/int_ref.py rounded to FP64), `<name>/sabs`
(the sum of absolute terms, each element's rounding scale) and `<name>/host` (the host FP64
path, int_cases.host_int2e); then the measured host error per total order L in units of
2^-53 sabs (`host_units`), kappa(L) = max(64, 8 x that) (`kappa`), and the same for
xt_eval_ao (`ao_host_units`, `ao_c`).  The entries are split over int_ref.npz, int_ref_2.npz, ... to keep
every file under 464 KB (int_cases.load_fixture reads them all).  It prints both tables; DESIGN.md records them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import int_cases as ic      # noqa: E402
import int_ref              # noqa: E402

OUT = os.path.join(HERE, "int_ref.npz")
SPLIT_BYTES = 440 * 1000        # uncompressed payload per file


def case_entry(c):
    """(ref, sabs, host, Lmap) of one case."""
    tb = ic.build(c)
    ref, sabs, Lmap = int_ref.ref_int2e(tb.pinfo, tb.pprim, tb.eab, tb.kinfo, tb.kprim, tb.ek, tb.omega,
                                        tb.nrow, tb.ldo)
    return ref, sabs, ic.host_int2e(tb), Lmap


def ao_measure():
    """Largest |host - ref| / (2^-53 sabs) of Mole.eval_ao (deriv = 1) over the AO test points,
    after the underflow allowance of int_ref.ao_bound."""
    from xtddft_amd.qc.dints import _sph_table, ao_shell_tables
    mol = ic.ao_mol()
    coords, _ = ic.ao_points()
    info, dat = ao_shell_tables(mol)
    ref, sabs, amp = int_ref.ref_eval_ao(coords, info, dat, _sph_table(), mol._norm, mol.nao)
    host = mol.eval_ao(coords, deriv=1).astype(int_ref.LD)
    excess = np.abs(host - ref) - int_ref.ao_bound(0.0, sabs, amp)
    live = sabs > 1e-290
    return float((excess[live] / (int_ref.LD(int_ref.U) * sabs[live])).max())


def main():
    d = {}
    measured = np.zeros(ic.L_MAX + 1)
    for c in ic.REF_CASES:
        ref, sabs, host, Lmap = case_entry(c)
        d[c.name + "/ref"], d[c.name + "/sabs"], d[c.name + "/host"] = ref, sabs, host
        measured = np.maximum(measured, ic.measured_ratio(host, ref, sabs, Lmap))
        print(c.name, ref.shape, flush=True)
    kappa = ic.kappa_from(measured)
    ao_units = ao_measure()
    ao_c = max(ic.AO_C_FLOOR, ic.AO_C_FACTOR * ao_units)
    head = dict(host_units=measured, kappa=kappa, ao_host_units=np.array(ao_units), ao_c=np.array(ao_c))
    # split so that no file passes the size of the largest fixture committed before (464 KB)
    files, cur, size = [], dict(head), 0
    for c in ic.REF_CASES:
        part = {k: d[k] for k in (c.name + "/ref", c.name + "/sabs", c.name + "/host")}
        nbytes = sum(v.nbytes + 300 for v in part.values())
        if size + nbytes > SPLIT_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur.update(part)
        size += nbytes
    files.append(cur)
    for old in ic.fixture_files():
        os.remove(old)
    for i, part in enumerate(files):
        np.savez_compressed(OUT if i == 0 else OUT.replace(".npz", f"_{i + 1}.npz"), **part)
    print("\n L   host error / (2^-53 sabs)   kappa(L)")
    for L in range(ic.L_MAX + 1):
        print(f"{L:2d}   {measured[L]:12.2f}              {kappa[L]:10.1f}")
    print(f"xt_eval_ao: host {ao_units:.2f} units, c = {ao_c:.1f}")
    for f in ic.fixture_files():
        print(f"{f}: {os.path.getsize(f)} bytes")
        assert os.path.getsize(f) <= ic.FIXTURE_MAX_BYTES


if __name__ == "__main__":
    main()
